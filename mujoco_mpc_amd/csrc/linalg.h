// linalg.h — small dense SPD factorisation / solves for one wavefront.
//
//  * generic (any n, also the 1-lane emulation build): A = L L^T, left-looking in LDS, one SYNC pair per column,
//    Linv[j] = 1/L[j][j];
//  * NVT > 0 (gfx950 only, n == NVT known at compile time): A = L^T D L with lane i keeping ROW i of the matrix in VGPRs;
//    pivots and rows are broadcast lane to lane (a 64-bit row DPP move where every consumer sits in the pivot's 16-lane row,
//    v_readlane otherwise: no LDS traffic, no waits on the pivot chain); the substitutions keep x in a VGPR per lane.
//    A factor/solve pair always uses the same form (the layouts in LDS differ).
// One wave per matrix is latency-bound, so the register form is several times faster than the LDS form.
#pragma once
#include <type_traits>
#include "dmath.h"
#include "model.h"

struct Ctx;

#ifndef MJPC_EMU
DEV double readlane_d(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// Every lane reads lane (K & 15) of ITS OWN 16-lane row: one v_mov_b64_dpp row_newbcast, no SGPR pair and none of the wait
// states between a v_readlane and the VALU instruction that consumes its SGPRs.  Needs full EXEC: a disabled source lane
// yields zero, not its value.  The register factorisations below are therefore called with all 64 lanes enabled (they sit
// between wave-uniform SYNCs) and mask their inactive lanes with `act ? ... : 0.0` selects, never with a divergent branch.
// bound_ctrl is set although a row broadcast has no out-of-range source: with it (and full row / bank masks) the compiler
// knows the old value of the destination is dead and does not zero the register pair ahead of every move.
template <int K>
DEV double rowbcast_d(double v) {
  return __longlong_as_double(__builtin_amdgcn_update_dpp((long long)0, __double_as_longlong(v), 0x150 + (K & 15), 0xf, 0xf, true));
}
// broadcast of lane K: within the rows when LOCAL says that no lane outside K's row uses the value (see below), to the wave otherwise
template <int K, bool LOCAL>
DEV double bcast_d(double v) {
  if constexpr (LOCAL) return rowbcast_d<K>(v);
  else return readlane_d(v, K);
}
#endif

// ---- generic LDS versions -----------------------------------------------------------------
DEV void chol_factor_lds(double *A, double *Linv, double *tmp, int n, int nvp) {
  for (int j = 0; j < n; j++) {
    SYNC();
    PFOR(ii, n - j) {
      int i = j + ii;
      double s = A[i * nvp + j];
#pragma unroll 4
      for (int k = 0; k < j; k++) s -= A[i * nvp + k] * A[j * nvp + k];
      tmp[i] = s;
    }
    SYNC();
    double t = tmp[j];
    if (t < D_MINVAL) t = D_MINVAL;
    double dj = sqrt(t), inv = 1.0 / dj;
    PFOR(ii, n - j) {
      int i = j + ii;
      A[i * nvp + j] = (i == j) ? dj : tmp[i] * inv;
    }
    if (LANE == 0) Linv[j] = inv;
  }
  SYNC();
}
DEV void chol_solve_lds(const double *L, const double *Linv, double *x, int n, int nvp) {
  for (int i = 0; i < n; i++) {
    SYNC();
    double xi = x[i] * Linv[i];
    SYNC();
    PFOR(kk, n - i - 1) { int k = i + 1 + kk; x[k] -= L[k * nvp + i] * xi; }
    if (LANE == 0) x[i] = xi;
  }
  for (int i = n - 1; i >= 0; i--) {
    SYNC();
    double xi = x[i] * Linv[i];
    SYNC();
    PFOR(k, i) x[k] -= L[i * nvp + k] * xi;
    if (LANE == 0) x[i] = xi;
  }
  SYNC();
}

// ---- register versions (compile-time n) -----------------------------------------------------
// A = L^T D L (L unit lower triangular, pivots taken from the last dof up, like MuJoCo's mj_factorM order).
// Lane i keeps the full symmetric row i in VGPRs.  A pivot step broadcasts 1/d_k and row k with v_readlane
// (SGPR operands of the trailing FMAs): no LDS traffic and no waits on the pivot chain, which is
//   readlane(d_k) -> rcp + 2 Newton steps -> l = a[k]*r -> d_{k-1} update;
// the rank-1 update of the other columns is independent work the scheduler overlaps with that chain.
// Afterwards lane i holds  up[k] = L[k][i] (k > i, else 0)  and  lo[j] = L[i][j] (j < i, else 0),
// so both substitutions are "broadcast + one FMA" per step.
//
// Row-local broadcasts keep the bits.  v_readlane hands lane k's value to all 64 lanes; rowbcast_d hands it to the lanes of
// k's row only, the lanes of the other rows receive the value of THEIR row's lane k & 15 instead.  It is used where every
// lane that multiplies the value by something non-zero lies in k's row (dense_up_local / dense_down_local here,
// tree_up_local / tree_down_local for the level order).  A lane of another row receives a different but finite value (a
// matrix entry, a positive reciprocal, a solution entry; 0.0 / 1.0 on inactive lanes) and multiplies it by a factor that is
// exactly zero there: l = (i < k) ? .. : 0.0, or an entry of L outside the pattern, a product of a structural +0 with a
// positive reciprocal.  The FMA then adds a zero to its accumulator: a non-zero accumulator is unchanged, and a +0 one stays
// +0 whatever the sign of the product, exactly as with the value v_readlane would have delivered.
template <int N> constexpr bool dense_up_local(int k) { return k < 16; }                               // consumers i < k: pivots 1..15, any N
template <int N> constexpr bool dense_down_local(int j) { return (j >> 4) == ((N - 1) >> 4); }         // consumers j < i < N
#ifndef MJPC_EMU
template <int N>
struct LDLRegs { double lo[N], up[N], rinv; };
// the matrix to factor may arrive as a sum: A plus up to three partial matrices of the same layout (the worker waves' partial
// Hessians, solver_reg.h); they are added while the rows are loaded
struct LDLExtra { const double *x[3]; int n; const double *row; };      // row != nullptr: lane i already holds the full symmetric row i of A in registers (A itself is not read)

template <int I, int E, class F>
DEV void static_for(F &&f) {
  if constexpr (I < E) { f(std::integral_constant<int, I>{}); static_for<I + 1, E>(f); }
}
// every index below is a compile-time constant (static_for, not `#pragma unroll`: with N = 33 the nested pragma loops exceeded
// the unroller's budget, the row array stayed in scratch memory and the kernel wrote gigabytes of spills per launch)
// row i of the symmetric matrix (only its lower triangle is valid in LDS) and its diagonal entry, partial matrices added
//
// Where lane i finds its row depends on the lane alone: entry j at (max(i, j), min(i, j)) of the lower triangle, the diagonal at
// (i, i).  The offsets are formed once and serve A and every partial (same layout, same stride).  The lane index is clamped once
// (an inactive lane, i >= N, walks column 0: entries (j, 0), inside the block and in the lower triangle), every lane loads and
// adds without a select, and ONE mask at the end gives the inactive lanes a[j] = +0.0 and dg = 1.0: what the row-local
// broadcasts of the factorisations need (finite operands beside their exact zeros, see above the dense routines; an inactive
// lane's sums are discarded by the select whatever they are).  An active lane forms ((A + X0) + X1) + X2 as before.
template <int N>
struct LDLRowOff { int e[N], d; };
template <int N>
DEV void ldl_row_offsets(int nvp, LDLRowOff<N> &o) {
  const int ic = LANE < N ? LANE : 0;
  static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; o.e[j] = (j <= ic) ? ic * nvp + j : j * nvp + ic; });
  o.d = ic * nvp + ic;
}
template <int N>
DEV void ldl_load_row(const double *A, int nvp, const LDLExtra *ex, double *a, double &dg) {
  const int i = LANE;
  const bool act = i < N;
  LDLRowOff<N> o;
  ldl_row_offsets<N>(nvp, o);
  if (ex && ex->row) {
    dg = 1.0;
    static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; a[j] = ex->row[j]; dg = (j == i) ? ex->row[j] : dg; });
  } else {
    static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; a[j] = A[o.e[j]]; });
    dg = A[o.d];
  }
  if (ex && ex->n > 0) {
    const int nx = ex->n;
    double t[3][N], td[3];
#pragma unroll
    for (int w = 0; w < 3; w++) {
      const double *X = ex->x[w < nx ? w : 0];
      static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; t[w][j] = X[o.e[j]]; });
      td[w] = X[o.d];
      if (w + 1 >= nx) break;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int w = 0; w < 3; w++) {
      if (w >= nx) break;
      static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; a[j] += t[w][j]; });
      dg += td[w];
    }
  }
  static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; a[j] = act ? a[j] : 0.0; });
  dg = act ? dg : 1.0;
}
// the elimination proper, from the row (and diagonal entry) ldl_load_row left in the lane's registers; a[] is consumed
template <int N>
DEV void ldl_eliminate_regs(double *a, double dg, LDLRegs<N> &f) {
  static_assert(N >= 1 && N <= 64, "one matrix row per lane");
  const int i = LANE;
  const bool act = i < N;
  static_for<1, N>([&](auto kc) {
    constexpr int k = N - decltype(kc)::value;                                 // N-1 ... 1
    constexpr bool loc = dense_up_local<N>(k);
    double rk = bcast_d<k, loc>(fast_rcp(dg < D_MINVAL ? D_MINVAL : dg));      // reciprocal in the vector domain, then broadcast
    double hk = a[k];
    double l = (i < k) ? hk * rk : 0.0;
    dg -= l * hk;
    // A[i][j] -= L[k][i] * A[k][j]: broadcast row k in groups of 8 first, then the FMAs, so that the SGPR written by a
    // v_readlane (or the VGPR a DPP move reads) is not touched by the very next VALU instruction (those hazards cost an
    // s_nop per update otherwise)
    static_for<0, (k + 7) / 8>([&](auto gc) {
      constexpr int j0 = decltype(gc)::value * 8;
      double sj[8];
      static_for<0, 8>([&](auto qc) { constexpr int q = decltype(qc)::value; if constexpr (j0 + q < k) sj[q] = bcast_d<k, loc>(a[j0 + q]); });
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, 8>([&](auto qc) { constexpr int q = decltype(qc)::value; if constexpr (j0 + q < k) a[j0 + q] -= l * sj[q]; });
      __builtin_amdgcn_sched_barrier(0);
    });
    f.up[k] = l;
  });
  f.up[0] = 0.0;
  if (dg < D_MINVAL) dg = D_MINVAL;
  f.rinv = fast_rcp(dg);
  static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; f.lo[j] = (act && j < i) ? a[j] * f.rinv : 0.0; });
}
template <int N>
DEV void ldl_factor_regs(const double *A, int nvp, LDLRegs<N> &f, const LDLExtra *ex = nullptr) {
  double a[N];
  double dg;
  ldl_load_row<N>(A, nvp, ex, a, dg);
  ldl_eliminate_regs<N>(a, dg, f);
}
template <int N>
DEV double ldl_solve_regs(const LDLRegs<N> &f, double xi) {
  static_for<1, N>([&](auto kc) { constexpr int k = N - decltype(kc)::value; xi -= f.up[k] * bcast_d<k, dense_up_local<N>(k)>(xi); });      // L^T u = b
  xi *= f.rinv;                                                                                                          // D v = u
  static_for<0, N - 1>([&](auto jc) { constexpr int j = decltype(jc)::value; xi -= f.lo[j] * bcast_d<j, dense_down_local<N>(j)>(xi); });      // L x = v
  return xi;
}
// ---- tree-structured elimination (DofTree<N>::known, DevModel::tree_ok) ----------------------------------------------
// Same L^T D L, same per-entry arithmetic, but (a) the pivots of one tree level (same height above the leaves: never
// related to each other) are processed together, so their reciprocal chains and trailing updates are independent work
// the scheduler interleaves, and (b) only the ancestors of a pivot are updated: the other columns of M's pattern are
// structural zeros.  Cross-branch contacts break the pattern of H; the caller then asks for the dense order.
template <int N> constexpr int tree_depth(int k) { int d = 0; for (int a = DofTree<N>::parent(k); a >= 0; a = DofTree<N>::parent(a)) d++; return d; }
template <int N> constexpr int tree_nth_anc(int k, int n) { int a = DofTree<N>::parent(k); for (int q = 0; q < n; q++) a = DofTree<N>::parent(a); return a; }
template <int N> constexpr int tree_height(int k) {
  int h = 0;
  for (int c = k + 1; c < N; c++) if (DofTree<N>::parent(c) == k) { int hc = tree_height<N>(c) + 1; if (hc > h) h = hc; }
  return h;
}
template <int N> constexpr int tree_nlevel() { int h = 0; for (int k = 0; k < N; k++) { int hk = tree_height<N>(k); if (hk > h) h = hk; } return h + 1; }   // forests: the tallest root
// (pivot, ancestor) pairs of one level, pivots in descending order
template <int N> constexpr int tree_level_npair(int H) { int n = 0; for (int k = N - 1; k >= 1; k--) if (tree_height<N>(k) == H) n += tree_depth<N>(k); return n; }
template <int N> constexpr int tree_level_pair(int H, int e, bool pivot) {
  for (int k = N - 1; k >= 1; k--) if (tree_height<N>(k) == H) {
    int d = tree_depth<N>(k);
    if (e < d) return pivot ? k : tree_nth_anc<N>(k, e);
    e -= d;
  }
  return 0;
}
// Row-local broadcasts (rowbcast_d, see the argument above the dense routines).  Pivot k's reciprocal, its row and its
// L^T u = b step are consumed by the ancestors of k only: local when all of them sit in k's 16-lane row.  Step j of L x = v
// is consumed by the descendants of j: local when all of those sit in j's row.
template <int N> constexpr bool tree_up_local(int k) { for (int a = DofTree<N>::parent(k); a >= 0; a = DofTree<N>::parent(a)) if ((a >> 4) != (k >> 4)) return false; return true; }
template <int N> constexpr bool tree_is_anc(int j, int c) { for (int a = DofTree<N>::parent(c); a >= 0; a = DofTree<N>::parent(a)) if (a == j) return true; return false; }
template <int N> constexpr bool tree_down_local(int j) { for (int c = j + 1; c < N; c++) if (tree_is_anc<N>(j, c) && (c >> 4) != (j >> 4)) return false; return true; }
template <int N> constexpr int tree_npair(bool local_only) { int n = 0; for (int k = 1; k < N; k++) if (!local_only || tree_up_local<N>(k)) n += tree_depth<N>(k); return n; }
template <int N> constexpr int tree_nup_local() { int n = 0; for (int k = 1; k < N; k++) n += tree_up_local<N>(k); return n; }
template <int N> constexpr int tree_ndown(bool local_only) { int n = 0; for (int j = 0; j < N; j++) if (tree_height<N>(j) > 0 && (!local_only || tree_down_local<N>(j))) n++; return n; }
// the quadruped (lane = dof): 84 of the 99 (pivot, ancestor) pairs are row-local, only the last two dofs of the fourth leg
// reach back across the row boundary; 7 of the 14 steps of L x = v
static_assert(tree_npair<18>(false) == 99 && tree_npair<18>(true) == 84, "DofTree<18>: row-local pairs");
static_assert(tree_nup_local<18>() == 15 && !tree_up_local<18>(16) && !tree_up_local<18>(17), "DofTree<18>: pivots 16 and 17 cross the row boundary");
static_assert(tree_ndown<18>(false) == 14 && tree_ndown<18>(true) == 7, "DofTree<18>: row-local steps of L x = v");
#define TREE_BAR() __builtin_amdgcn_sched_barrier(0)
template <int N>
DEV void ldl_eliminate_tree(double *a, double dg, LDLRegs<N> &f) {
  static_assert(DofTree<N>::known && N <= 64, "one matrix row per lane");
  const int i = LANE;
  const bool act = i < N;
  static_for<0, tree_nlevel<N>()>([&](auto hc) {
    constexpr int H = decltype(hc)::value;
    // 1/d in the vector domain (every lane inverts its own diagonal: one reciprocal chain per LEVEL, no scalar clamp
    // round trip), then the pivots' reciprocals are broadcast
    const double rv = fast_rcp(dg < D_MINVAL ? D_MINVAL : dg);
    static_for<1, N>([&](auto kc) {
      constexpr int k = N - decltype(kc)::value;
      if constexpr (tree_height<N>(k) == H) f.up[k] = bcast_d<k, tree_up_local<N>(k)>(rv);
    });
    static_for<1, N>([&](auto kc) {                       // l = L[k][i] on the ancestors of k, diagonal update
      constexpr int k = N - decltype(kc)::value;
      if constexpr (tree_height<N>(k) == H) {
        double hk = a[k];
        double l = (i < k) ? hk * f.up[k] : 0.0;
        dg -= l * hk;
        f.up[k] = l;
      }
    });
    constexpr int NP = tree_level_npair<N>(H);            // A[i][j] -= L[k][i] * A[k][j], j ancestor of k
    constexpr int CHUNK = 8;                              // pairs fetched (broadcast) ahead of their updates
    static_for<0, (NP + CHUNK - 1) / CHUNK>([&](auto gc) {
      constexpr int e0 = decltype(gc)::value * CHUNK;
      double sj[CHUNK];
      static_for<0, CHUNK>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if constexpr (e0 + q < NP) {
          constexpr int j = tree_level_pair<N>(H, e0 + q, false), k = tree_level_pair<N>(H, e0 + q, true);
          sj[q] = bcast_d<k, tree_up_local<N>(k)>(a[j]);
        }
      });
      TREE_BAR();
      static_for<0, CHUNK>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if constexpr (e0 + q < NP) {
          constexpr int j = tree_level_pair<N>(H, e0 + q, false), k = tree_level_pair<N>(H, e0 + q, true);
          a[j] -= f.up[k] * sj[q];
        }
      });
      TREE_BAR();
    });
  });
  f.up[0] = 0.0;
  if (dg < D_MINVAL) dg = D_MINVAL;
  f.rinv = fast_rcp(dg);
#pragma unroll
  for (int j = 0; j < N; j++) f.lo[j] = (act && j < i) ? a[j] * f.rinv : 0.0;
}
template <int N>
DEV void ldl_factor_tree(const double *A, int nvp, LDLRegs<N> &f, const LDLExtra *ex = nullptr) {
  double a[N];
  double dg;
  ldl_load_row<N>(A, nvp, ex, a, dg);
  ldl_eliminate_tree<N>(a, dg, f);
}
template <int N>
DEV double ldl_solve_tree(const LDLRegs<N> &f, double xi) {
  static_for<0, tree_nlevel<N>()>([&](auto hc) {          // L^T u = b, leaves first
    constexpr int H = decltype(hc)::value;
    double s[N];
    static_for<1, N>([&](auto kc) { constexpr int k = N - decltype(kc)::value; if constexpr (tree_height<N>(k) == H) s[k] = bcast_d<k, tree_up_local<N>(k)>(xi); });
    static_for<1, N>([&](auto kc) { constexpr int k = N - decltype(kc)::value; if constexpr (tree_height<N>(k) == H) xi -= f.up[k] * s[k]; });
  });
  xi *= f.rinv;                                           // D v = u
  static_for<1, tree_nlevel<N>()>([&](auto hc) {          // L x = v, root first (leaves have no descendants)
    constexpr int H = tree_nlevel<N>() - decltype(hc)::value;
    double s[N];
    static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; if constexpr (tree_height<N>(j) == H) s[j] = bcast_d<j, tree_down_local<N>(j)>(xi); });
    static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; if constexpr (tree_height<N>(j) == H) xi -= f.lo[j] * s[j]; });
  });
  return xi;
}
template <int N>
DEV void ldl_factor_any(const double *A, int nvp, LDLRegs<N> &f, int tree, const LDLExtra *ex = nullptr) {
  if constexpr (DofTree<N>::known) { if (tree) { ldl_factor_tree<N>(A, nvp, f, ex); return; } }
  ldl_factor_regs<N>(A, nvp, f, ex);
}
template <int N>
DEV double ldl_solve_any(const LDLRegs<N> &f, double xi, int tree) {
  if constexpr (DofTree<N>::known) { if (tree) return ldl_solve_tree<N>(f, xi); }
  return ldl_solve_regs<N>(f, xi);
}
// split form (factor kept in LDS between phases): L[i][j] (j < i) in the lower triangle of A, 1/d in Dinv
template <int N>
DEV void chol_factor_reg(double *A, double *Dinv, int nvp, int tree) {
  SYNC();
  LDLRegs<N> f;
  ldl_factor_any<N>(A, nvp, f, tree);
  const int i = LANE;
  static_for<0, N>([&](auto jc) { constexpr int j = decltype(jc)::value; if (i < N && j < i) A[i * nvp + j] = f.lo[j]; });
  if (i < N) Dinv[i] = f.rinv;
  SYNC();
}
template <int N>
DEV void chol_solve_reg(const double *L, const double *Dinv, double *x, int nvp, int tree) {
  SYNC();
  const int i = LANE;
  const bool act = i < N;
  LDLRegs<N> f;
  f.rinv = act ? Dinv[i] : 0.0;
  // lo[k] and up[k] are never both set: one load per k, entry (max(i, k), min(i, k)) as in ldl_load_row (k == i reads the diagonal
  // slot, which the factor leaves alone, and drops it)
  LDLRowOff<N> o;
  ldl_row_offsets<N>(nvp, o);
  static_for<0, N>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const double v = L[o.e[k]];
    f.lo[k] = (act && k < i) ? v : 0.0;
    f.up[k] = (act && k > i) ? v : 0.0;
  });
  double xi = ldl_solve_any<N>(f, act ? x[i] : 0.0, tree);
  if (act) x[i] = xi;
  SYNC();
}
// fused factor + solve (the factor never leaves the registers): Newton direction, implicit-damping solve.
// negx: also receives -x (the Newton solver's search direction, from the lane that holds the solution entry)
template <int N>
DEV void chol_factor_solve_reg(const double *A, double *x, int nvp, int tree, const LDLExtra *ex = nullptr, double *negx = nullptr) {
  SYNC();
  LDLRegs<N> f;
  ldl_factor_any<N>(A, nvp, f, tree, ex);
  const int i = LANE;
  double xi = ldl_solve_any<N>(f, i < N ? x[i] : 0.0, tree);
  if (i < N) { x[i] = xi; if (negx) negx[i] = -xi; }
  SYNC();
}
#endif

// `tree`: the matrix has the sparsity pattern of M and the model's dof tree is DofTree<NVT> (DevModel::tree_ok)
template <int NVT>
DEV void chol_factor(double *A, double *Linv, double *tmp, int n, int nvp, int tree) {
#ifndef MJPC_EMU
  if constexpr (NVT > 0) { chol_factor_reg<NVT>(A, Linv, NVP_OF(NVT), tree); return; }
#endif
  chol_factor_lds(A, Linv, tmp, n, nvp);
}
template <int NVT>
DEV void chol_solve(const double *L, const double *Linv, double *x, int n, int nvp, int tree) {
#ifndef MJPC_EMU
  if constexpr (NVT > 0) { chol_solve_reg<NVT>(L, Linv, x, NVP_OF(NVT), tree); return; }
#endif
  chol_solve_lds(L, Linv, x, n, nvp);
}
// A (lower triangle) is consumed; x <- A^-1 x.  The generic build leaves the LL^T factor in A / Linv.
template <int NVT>
DEV void chol_factor_solve(double *A, double *Linv, double *tmp, double *x, int n, int nvp, int tree) {
#ifndef MJPC_EMU
  if constexpr (NVT > 0) { chol_factor_solve_reg<NVT>(A, x, NVP_OF(NVT), tree); return; }
#endif
  chol_factor_lds(A, Linv, tmp, n, nvp);
  chol_solve_lds(A, Linv, x, n, nvp);
}
