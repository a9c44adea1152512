// gradient.h — device side of the Sample-Gradient planner (mjpc/planners/sample_gradient/planner.cc) besides the rollouts:
//   sg_assemble   the mixed candidate table of one plan step (planner.cc:357-398): un-noised nominal, noisy candidates,
//                 explicit policies; plus the persistent noise history that stands in for the reference's `noise` vector
//                 (planner.cc:94, 339-344)
//   sg_produce / sg_consume   gradient[k] = sum_i hist[slot[i]][k] * scale[i] (planner.cc:452-459), every product rounded,
//                 then added in ascending i: the reference's mju_addToScl loop bit for bit
// The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_gradient.cpp) runs the same functions
// one after the other in a single thread.
#pragma once
#include <stddef.h>
#include "spmd.h"
#include "dmath.h"

// ------------------------------------------------------------------------------ batch assembly
struct SgAssembleArgs {
  const double *nominal;      // [PN] nominal knot values
  const double *noise_std;    // [PN] absolute per-parameter std
  const double *eps;          // [nlocal][PN] standard normals of this plan
  const double *ctrlrange;    // [2 * nu]
  double *cand;               // [nlocal][PN] candidate table; rows >= first_explicit hold the caller's knots already
  double *hist;               // [max_local][hist_stride] noise history, slot = local row
  long long hist_stride;      // P_max * nu
  int offset, nlocal, PN, nu, nominal_index, first_explicit;
};

// element idx = r * PN + e of the table.  Noisy rows repeat ph_init's Cross-Entropy branch (core.h) with the same helpers in the
// same order, so a mixed plan's rows below first_explicit are bit for bit those of a plain plan with noise_std.  The history
// takes eps only for rows nominal_index < global index < first_explicit and only in [0, PN): slot 0, the explicit slots and
// the tail beyond PN keep what an earlier plan left there (the reference's behaviour when its sliders move).
DEV void sg_assemble(const SgAssembleArgs &a, size_t idx) {
  int r = (int)(idx / (size_t)a.PN), e = (int)(idx - (size_t)r * a.PN);
  int gi = a.offset + r;
  if (gi >= a.first_explicit) return;
  double v = a.nominal[e];
  if (gi != a.nominal_index) {
    int k = e % a.nu;
    double lo = a.ctrlrange[2 * k], hi = a.ctrlrange[2 * k + 1];
    double eps = a.eps[idx];
    v = add_mul3_rn(v, 1.0, a.noise_std[e], eps);
    v = d_clip(v, lo, hi);
    if (gi > a.nominal_index) a.hist[(size_t)r * a.hist_stride + e] = eps;
  }
  a.cand[idx] = v;
}

// ------------------------------------------------------------------------------ gradient reduction
// One workgroup owns SG_KT parameters.  The add chain of a parameter is serial by definition (n dependent fp64 adds), so the
// HBM loads are kept off it: producer threads (SG_PROD groups of SG_KT lanes) fetch SG_U history rows each - all in flight at
// once - round the products and stage them in a tile of SG_T rows; the SG_KT consumer lanes add a finished tile from there in
// row order while the producers fill the other tile.  The result does not depend on how rows are dealt to producers.
#define SG_KT 16
#define SG_U 16
#define SG_PROD 12
#define SG_T (SG_U * SG_PROD)

struct SgGradArgs {
  const double *hist; long long hist_stride;
  const int *slot;            // [n] history slots, each in [0, max_local) (checked on the host)
  const double *scale;        // [n]
  int n, PN;
  double *gradient;           // [PN]
};

// producer group g (0 .. SG_PROD-1), parameter lane kl of k-block kb: rows tile * SG_T + u * SG_PROD + g of the tile
DEV void sg_produce(const SgGradArgs &a, int kb, int tile, int g, int kl, double *buf) {
  int k = kb * SG_KT + kl;
  if (k >= a.PN) return;
  int i0 = tile * SG_T;
  // rows behind the last one load row n - 1 again (n >= 1) and stage a product nobody adds: no branch between the loads, so
  // all SG_U of them are in flight together
  int sl[SG_U];
  double sc[SG_U], v[SG_U];
#pragma unroll
  for (int u = 0; u < SG_U; u++) {
    int i = i0 + u * SG_PROD + g;
    if (i > a.n - 1) i = a.n - 1;
    sl[u] = a.slot[i]; sc[u] = a.scale[i];
  }
#pragma unroll
  for (int u = 0; u < SG_U; u++) v[u] = a.hist[(size_t)sl[u] * a.hist_stride + k];
#pragma unroll
  for (int u = 0; u < SG_U; u++) buf[(u * SG_PROD + g) * SG_KT + kl] = mul_rn(v[u], sc[u]);
}

// consumer lane kl: acc += the tile's products in ascending row order, one rounded add each
DEV double sg_consume(const SgGradArgs &a, int tile, int kl, const double *buf, double acc) {
  int rows = a.n - tile * SG_T;
  if (rows > SG_T) rows = SG_T;
#pragma unroll 8
  for (int j = 0; j < rows; j++) acc = add_rn(acc, buf[j * SG_KT + kl]);
  return acc;
}
