// tests/emu/emu_cost_derivatives.cpp — TEST INFRASTRUCTURE ONLY.
// The cost-derivative and backward-recursion kernels (mujoco_mpc_amd/csrc/cost_derivatives.h) in the 1-lane emulation mode:
// emu_cost_derivatives plays cd_kernel (engine.hip) workgroup by workgroup and thread by thread in the kernel's phase order, through a
// NaN-poisoned LDS image, onto the caller's (NaN-poisoned) outputs, so that an entry stored without having been computed, or never
// stored, shows up; emu_gradient_backward plays gd_backward_kernel.  Never loaded by the product.
#define MJPC_EMU 1
#include <vector>
#include "../../mujoco_mpc_amd/csrc/cost_derivatives.h"
#include "../../include/mjpc_hip.h"

extern "C" int emu_cost_derivatives(const MjpcHipTask *task, int T, int nd, int nu, const double *residual, const double *C, const double *D,
                                    int last_is_terminal, int hessians, double *cr, double *cx, double *cu, double *cxx, double *cuu, double *cxu) {
  CdArgs a;
  a.residual = residual; a.C = C; a.D = D;
  a.dim_norm_residual = task->dim_norm_residual; a.norm = task->norm; a.num_norm_parameter = task->num_norm_parameter;
  a.weight = task->weight; a.norm_parameter = task->norm_parameter; a.num_term = task->num_term; a.risk = task->risk;
  a.T = T; a.nd = nd; a.nu = nu; a.nr = task->num_residual; a.last_is_terminal = last_is_terminal ? 1 : 0; a.hessians = hessians ? 1 : 0;
  a.cr = cr; a.cx = cx; a.cu = cu; a.cxx = cxx; a.cuu = cuu; a.cxu = cxu;
  const int n = nd + nu, NT = CD_TILE * CD_TILE, tiles = (n + CD_TILE - 1) / CD_TILE;
  const double nan = 0.0 / 0.0;
  std::vector<double> sm(CD_LDS_DOUBLES(a.nr, a.num_term));
  for (int t = 0; t < T; t++)
    for (int by = 0; by < (a.hessians ? tiles : 1); by++)
      for (int bx = 0; bx < tiles; bx++) {
        for (auto &v : sm) v = nan;
        const CdLds L = cd_lds(a, sm.data());
        const int i0 = by * CD_TILE, j0 = bx * CD_TILE;
        for (int k = 0; k < a.num_term; k++) cd_term(a, t, k, L);
        const double s = cd_risk_scale(a, L);
        for (int tid = 0; tid < (a.hessians ? 2 : 1) * CD_TILE; tid++) {
          const int j = tid < CD_TILE ? j0 + tid : i0 + (tid - CD_TILE);
          L.gv[tid] = j < n ? cd_gradient(a, t, j, L, s) : 0.0;
        }
        if (bx == 0 && by == 0 && a.cr) for (int r = 0; r < a.nr; r++) a.cr[(size_t)t * a.nr + r] = L.cr[r];
        if (by == 0)
          for (int tid = 0; tid < CD_TILE && j0 + tid < n; tid++) {
            const int j = j0 + tid;
            if (j < nd) { if (a.cx) a.cx[(size_t)t * nd + j] = L.gv[tid]; }
            else if (a.cu) a.cu[(size_t)t * nu + (j - nd)] = L.gv[tid];
          }
        if (!a.hessians) continue;
        const int term = cd_terminal(a, t);
        if (term && bx == 0 && by == 0)
          for (size_t e = 0; e < (size_t)(nd > nu ? nd : nu) * nu; e++) { cd_zero_terminal(a, 0, e); cd_zero_terminal(a, 1, e); }
        if (i0 >= nd && j0 + CD_TILE <= nd) continue;
        std::vector<double> acc(NT, 0.0);
        int fs = 0;
        for (int k = 0; k < a.num_term; k++) {
          const int ni = a.dim_norm_residual[k], dense = norm_dense(a.norm[k]);
          if (dense)
            for (int idx = 0; idx < ni * CD_TILE; idx++) {
              const int c = j0 + idx % CD_TILE;
              L.S[idx] = (c < n && !(term && c >= nd)) ? cd_S_dense(a, t, k, fs, ni, idx / CD_TILE, c, L) : 0.0;
            }
          for (int tid = 0; tid < NT; tid++) {
            const int jj = tid % CD_TILE, ii = tid / CD_TILE;
            if (cd_dest(a, t, i0 + ii, j0 + jj)) acc[tid] = add_rn(acc[tid], mul_rn(cd_weight(a, k), cd_G(a, t, fs, ni, dense, i0 + ii, j0 + jj, jj, L)));
          }
          fs += ni;
        }
        for (int tid = 0; tid < NT; tid++) {
          const int jj = tid % CD_TILE, ii = tid / CD_TILE;
          double *dst = cd_dest(a, t, i0 + ii, j0 + jj);
          if (dst) *dst = cd_risk_entry(a, acc[tid], L.gv[CD_TILE + ii], L.gv[jj], s);
        }
      }
  return 0;
}

extern "C" int emu_gradient_backward(int T, int nd, int nu, const double *A, const double *B, const double *cx, const double *cu, double *k, double *Vx,
                                     double *Qx, double *Qu, double *dV) {
  if (T < 2) return -1;
  GdArgs a;
  a.A = A; a.B = B; a.cx = cx; a.cu = cu; a.T = T; a.nd = nd; a.nu = nu; a.k = k; a.Vx = Vx; a.Qx = Qx; a.Qu = Qu; a.dV = dV;
  const int n = nd + nu, nb = nd * n;
  const double nan = 0.0 / 0.0;
  const bool staged = gd_staged(a);
  std::vector<double> sm(2 * (size_t)n + (staged ? nb : 0), nan), next(staged ? nb : 0, nan);
  double *vx[2] = {sm.data(), sm.data() + nd}, *qu[2] = {sm.data() + 2 * nd, sm.data() + 2 * nd + nu};
  double *blk = staged ? sm.data() + 2 * n : nullptr;
  for (int c = 0; c < nd; c++) { const double v = cx[(size_t)(T - 1) * nd + c]; vx[0][c] = v; Vx[(size_t)(T - 1) * nd + c] = v; }
  if (staged) for (int i = 0; i < nb; i++) blk[i] = gd_block(a, T - 1, i);
  double dv = 0;
  for (int t = T - 1; t > 0; t--) {
    const int b = (T - 1 - t) & 1;
    if (staged && t > 1) for (int i = 0; i < nb; i++) next[i] = gd_block(a, t - 1, i);      // the threads' registers
    for (int c = 0; c < n; c++) {
      const double q = gd_column(a, t, c, vx[b], blk);
      if (c < nd) { Qx[(size_t)(t - 1) * nd + c] = q; Vx[(size_t)(t - 1) * nd + c] = q; vx[b ^ 1][c] = q; }
      else {
        const int kk = c - nd;
        Qu[(size_t)(t - 1) * nu + kk] = q; k[(size_t)(t - 1) * nu + kk] = -q; qu[b][kk] = q;
        if (t == T - 1) k[(size_t)(T - 1) * nu + kk] = -q;
      }
    }
    dv = gd_dv(a, qu[b], dv);
    if (staged && t > 1) for (int i = 0; i < nb; i++) blk[i] = next[i];
  }
  dV[0] = dv; dV[1] = 0.0;
  return 0;
}
