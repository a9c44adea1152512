// spmd.h — execution-model shim for the rollout engine.
//
// Product build (hipcc, gfx950): one workgroup of MJPC_WAVES = 4 64-lane wavefronts owns one candidate rollout, each wave in
// its own role (below); per-candidate mjData-like state lives in LDS; `PFOR` is a lane-strided loop over the lanes of ONE
// wave, `SYNC` orders that wave's memory traffic, `XBAR` is the workgroup barrier between the roles and flag_set / flag_wait the
// point-to-point hand-shake between two of them (slots of misc[], model.h); reductions / scans use cross-lane operations.
//
// MJPC_EMU build (g++, tests only): NLANE = 1 and one thread plays the owner and the side wave in turn (no helpers,
// MJPC_HELPER == 0): the same source runs as plain sequential C++ so that the CPU test tier can exercise the kernel
// logic (indexing, formulas) before a GPU run.
// The emu library is never loaded by the product (mujoco_mpc_amd/capi.py loads libmjpc_hip.so only).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef MJPC_EMU
#define DEV static inline
#define DEV_NOINLINE static
#define LANE 0
#define NLANE 1
#define SYNC() ((void)0)
// the emulation runs the owner's and the side wave's phases of a candidate one after the other in a single thread
#define MJPC_HELPER 0
#define XBAR() ((void)0)
#define ROLE0 1
#define ROLE1 1
#define ROLEH 0
DEV void flag_set(int *p, int v) { *p = v; }
DEV int flag_wait(int *p, int v) { return *p == v; }
DEV int flag_wait_ge(int *p, int v) { return *p >= v; }
DEV double mul_rn(double a, double b) { return a * b; }   // emu is built with -ffp-contract=off
DEV double add_rn(double a, double b) { return a + b; }
DEV double add_mul3_rn(double a, double b, double c, double d) { return a + (b * c) * d; }
DEV double wave_sum(double v) { return v; }
DEV void wave_sum3(double &a, double &b, double &c) {}
DEV void wave_sum4(double &a, double &b, double &c, double &d) {}
DEV double wave_min(double v) { return v; }
DEV int wave_sum_i(int v) { return v; }
DEV int wave_or_i(int v) { return v; }
DEV int wave_excl_scan(int v, int *total) { *total = v; return 0; }
DEV int wave_flag_scan(int flag, int *total) { *total = flag ? 1 : 0; return 0; }
DEV int wave_any(int flag) { return flag != 0; }
#else
#include <hip/hip_runtime.h>
#define DEV static __device__ __forceinline__
#define DEV_NOINLINE static __device__ __noinline__
// A candidate is owned by the four wavefronts of one workgroup, one per SIMD of a CU:
//   owner (wave 0, ROLE0): the serial critical path (kinematics -> collision / contact rows -> Newton solver -> integration);
//   helper 0 (wave 1): joint-space inertia and its factor while the owner builds the constraints, then the Jacobian rows of the
//     second half of the step's contacts (the owner fills the first half); during the solve the line search's records, then
//     cone-block jobs of the owner's Newton iterations (elliptic models, solver_reg.h);
//   helper 1 (wave 2): site positions and actuator forces, the contact-free constraint rows and half of the subtree sums; during
//     the solve the price of the unconstrained acceleration, then cone-block jobs;
//   side wave (wave 3, ROLE1): work that only hangs off that path (smooth dynamics while the owner builds the constraints;
//     residual / cost / trajectory record and the integrator's factor while the owner solves).
// SYNC() orders LDS traffic inside ONE wave (DS operations of a wave execute in order; only the compiler must not
// reorder them), XBAR() is the workgroup barrier between the roles.
// The spill flavour (rollout_spill.hip) keeps some of the same state in a per-candidate HBM slab, accessed with global / flat
// instructions, and relies on the same fences to order it (LLVM AMDGPU memory model, GFX942 family, which gfx950 follows):
//  - one wave: vector memory operations of a wave complete in issue order and a load sees the wave's earlier store to the
//    same address, so a wavefront-scope fence needs no wait instruction; the fence in SYNC() has no address space attached, so
//    it also stops the compiler from moving a global access across it.
//  - waves of the workgroup: without threadgroup-split mode (never enabled here) all waves of a workgroup run on one CU and
//    share its vector L1, so workgroup scope needs no cache invalidation; a workgroup-scope release (XBAR(), flag_set) waits
//    for the wave's earlier vector memory operations (s_waitcnt vmcnt) before the barrier / flag store, the acquire after it
//    keeps the later loads behind it.  Checked in the flavour's ISA: every s_barrier follows a vmcnt wait or the return of a
//    call (which drains all counters).
#define MJPC_WAVES 4
#define MJPC_NH 2            // helper waves (ROLEH)
#define MJPC_HELPER 1        // this is not the emulation: the helper waves exist
#define LANE ((int)(threadIdx.x & 63))
#define NLANE 64
#define SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define XBAR() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
#define WAVE_ID() (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)))
#define ROLE0 (WAVE_ID() == 0)
#define ROLE1 (WAVE_ID() == MJPC_WAVES - 1)
#define ROLEH (WAVE_ID() >= 1 && WAVE_ID() < MJPC_WAVES - 1)     // helper k = WAVE_ID() - 1
// individually rounded ops (no FMA contraction): used where results must be bit-identical to the CPU path
DEV double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
DEV double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
// a + (b*c)*d with every operation rounded separately
DEV double add_mul3_rn(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  double t = b * c;
  double u = t * d;
  return a + u;
}
// butterfly inside each row of 16 lanes with DPP moves (VALU rate), then the 4 row sums through readlane
DEV double dpp_xchg(double v, const int ctrl_sel) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  switch (ctrl_sel) {
    case 0: lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true); break;   // quad_perm [1,0,3,2]
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true); break;   // quad_perm [2,3,0,1]
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, true); break; // row_half_mirror
    case 3: lo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xF, 0xF, true); break; // row_mirror
    case 4: lo = __builtin_amdgcn_update_dpp(0, lo, 0x124, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x124, 0xF, 0xF, true); break; // row_ror:4
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xF, 0xF, true); break; // row_ror:8
  }
  return __hiloint2double(hi, lo);
}
// the four row sums (identical in every lane of a row after the butterflies) -> wave total: row_bcast:15 adds row 0 into
// row 1 and row 2 into row 3, row_bcast:31 adds row 1 into rows 2 / 3; lane 63 then holds (r3 + r2) + (r1 + r0), the same
// value as (r0 + r1) + (r2 + r3)
DEV double row_total(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  double t = __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x142, 0xA, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xA, 0xF, false));
  v += t;
  lo = __double2loint(v); hi = __double2hiint(v);
  t = __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x143, 0xC, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xC, 0xF, false));
  v += t;
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
DEV double wave_sum(double v) {
  v += dpp_xchg(v, 0);
  v += dpp_xchg(v, 1);
  v += dpp_xchg(v, 2);
  v += dpp_xchg(v, 3);
  // every lane of a row now holds that row's sum (the butterflies are symmetric => identical bits in all lanes)
  return row_total(v);
}
// Several reductions at once, TRANSPOSED: the sums share one register from the second tree level on, so a level costs one
// exchange and one add whatever the number of sums (one butterfly chain per sum costs 26 instructions per sum).
// The tree of every sum is wave_sum's, add for add; only the LANE that performs an add differs, and a + b == b + a in every bit
// (IEEE 754; a NaN result may carry either operand's payload), so no bit of a finite or infinite result moves:
//   level 1 (xor 1)  even lanes keep a and get the neighbour's a, odd lanes keep b and get the neighbour's b: one exchange of
//                    the value NOT kept, one add; lane l then holds the PAIR sum a[l] + a[l^1] (l even) or b[l] + b[l^1] (l odd),
//                    the pair sums wave_sum forms in both lanes of the pair.  The third (and fourth) value pair up likewise;
//   level 2 (xor 2)  the same one level up, pair register against pair register: lanes 0, 1 of a quad keep x, lanes 2, 3 keep y.
//                    Lane j of quad q now holds sum number j's QUAD sum Q_j[q] (three sums: lanes 2 and 3 both hold the third's);
//   levels 3, 4      wave_sum adds the two quads of an octet (row_half_mirror), then the two octets of a row (row_mirror); either
//                    mirror would move lane j to lane 3 - j of its quad.  row_ror:4 / row_ror:8 (lane l reads lane l - 4 / l - 8
//                    of its row, mod 16) keep j.  After ror:4 quad q holds Q[q] + Q[q-1]: an octet sum of the tree for q = 1
//                    (Q1 + Q0) and q = 3 (Q3 + Q2), a sum the tree never forms for q = 0, 2.  After ror:8 quad q adds quad q - 2:
//                    quads 1 and 3 hold (Q1 + Q0) + (Q3 + Q2) resp. (Q3 + Q2) + (Q1 + Q0), the row sum R of the tree, quads 0
//                    and 2 a differently associated one.  From here on ONLY lanes 4..7 and 12..15 of each row count;
//   levels 5, 6      v_permlane16_swap of (v, v) leaves rows {0, 0, 2, 2} of v in one result and rows {1, 1, 3, 3} in the other
//                    (rows of 16 lanes, lane positions kept): their sum is R0 + R1 in rows 0, 1 and R2 + R3 in rows 2, 3, the two
//                    adds of row_bcast:15.  v_permlane32_swap does the same with the halves: (R0 + R1) + (R2 + R3) in every
//                    row, the add of row_bcast:31.  Neither needs the zero-filled `old` operand of a row_bcast;
//   result           sum j from lane 12 + j (the lanes 4 + j and 12 + j of every row hold it).
// Requires full EXEC, as wave_sum does.
DEV double swap_add16(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
DEV double swap_add32(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
DEV double lane_value(double v, const int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// levels 3 .. 6 on the shared register
DEV double wave_sum_upper(double v) {
  v += dpp_xchg(v, 4);
  v += dpp_xchg(v, 5);
  v = swap_add16(v);
  return swap_add32(v);
}
DEV void wave_sum3(double &a, double &b, double &c) {
  const bool e1 = !(LANE & 1), e2 = !(LANE & 2);
  const double x = (e1 ? a : b) + dpp_xchg(e1 ? b : a, 0);
  const double y = c + dpp_xchg(c, 0);
  const double v = wave_sum_upper((e2 ? x : y) + dpp_xchg(e2 ? y : x, 1));
  a = lane_value(v, 12); b = lane_value(v, 13); c = lane_value(v, 14);
}
DEV void wave_sum4(double &a, double &b, double &c, double &d) {
  const bool e1 = !(LANE & 1), e2 = !(LANE & 2);
  const double x = (e1 ? a : b) + dpp_xchg(e1 ? b : a, 0);
  const double y = (e1 ? c : d) + dpp_xchg(e1 ? d : c, 0);
  const double v = wave_sum_upper((e2 ? x : y) + dpp_xchg(e2 ? y : x, 1));
  a = lane_value(v, 12); b = lane_value(v, 13); c = lane_value(v, 14); d = lane_value(v, 15);
}
DEV double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { double w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// OR over the 64 lanes on the VALU (the shuffle form is six dependent LDS round trips): butterflies inside each row, then the
// row_bcast steps of row_total; lane 63 has seen every lane.  Requires full EXEC.
DEV int wave_or_i(int v) {
  v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
  v |= __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
  return __builtin_amdgcn_readlane(v, 63);
}
DEV int wave_any(int flag) { return __builtin_amdgcn_ballot_w64(flag != 0) != 0; }
// point-to-point hand-shake between two waves of the workgroup through a sequence number in LDS: the setter publishes all
// its earlier LDS writes (release), the waiter spins (bounded: a protocol bug must not hang the GPU) and then acquires
DEV void flag_set(int *p, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (LANE == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
DEV int flag_wait(int *p, int v) {
  int ok = 0;
  for (int n = 0; n < (1 << 21); n++) {
    int cur = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (cur == v) { ok = 1; break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return ok;
}
// the same for a monotonically increasing sequence number: returns once *p >= v (a waiter that was late for v still gets through)
DEV int flag_wait_ge(int *p, int v) {
  int ok = 0;
  for (int n = 0; n < (1 << 21); n++) {
    int cur = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (cur >= v) { ok = 1; break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return ok;
}
// exclusive prefix sum over the 64 lanes (lane order), total returned to every lane: Hillis-Steele inside each
// row of 16 with DPP row_shr (VALU rate, zero fill), then row_bcast:15 / row_bcast:31 carry the row totals
DEV int wave_excl_scan(int v, int *total) {
  int x = v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);
  *total = __builtin_amdgcn_readlane(x, 63);
  return x - v;
}
// the same for 0/1 flags: ballot + popcount of the lower lanes
DEV int wave_flag_scan(int flag, int *total) {
  unsigned long long m = __builtin_amdgcn_ballot_w64(flag != 0);
  *total = __builtin_popcountll(m);
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
#endif

#define PFOR(i, n) for (int i = LANE; i < (n); i += NLANE)
