// tests/host/riccati_main.cpp — TEST INFRASTRUCTURE ONLY.
// The host side of the iLQG backward pass (BoxQPSolve, iLQGBackwardPass of csrc/planner.cc) in a stand-alone program that the test builds with
// the address and undefined-behaviour sanitizers: a box-QP at the humanoid's control count, a backward pass at the humanoid's dimensions
// (54, 21, 4) with and without limits, through both host entry points, and a pass whose control solve fails at one knot until the
// regularisation has grown.  Prints "riccati ok".  The engine calls planner.cc refers to are never made here and are left unresolved.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mjpc_hip_planner.h"

namespace {
unsigned long long g_state = 0x9E3779B97F4A7C15ull;
double Uniform() {          // in (-1, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_state >> 11) / 9007199254740992.0) * 2.0 - 1.0;
}
struct Problem {
  int n, m, T;
  std::vector<double> A, B, cx, cu, cxx, cxu, cuu, actions, limits;
};
// cost Hessians J'J / rows of a random Jacobian with more rows than columns: positive definite
Problem Random(int n, int m, int T) {
  Problem p;
  p.n = n; p.m = m; p.T = T;
  const int w = n + m, rows = w + 2;
  p.A.resize((size_t)(T - 1) * n * n); p.B.resize((size_t)(T - 1) * n * m);
  for (double& v : p.A) v = Uniform() / std::sqrt((double)n);
  for (double& v : p.B) v = Uniform() / std::sqrt((double)n);
  p.cx.resize((size_t)T * n); p.cu.resize((size_t)T * m);
  for (double& v : p.cx) v = Uniform();
  for (double& v : p.cu) v = Uniform();
  p.cxx.assign((size_t)T * n * n, 0.0); p.cxu.assign((size_t)T * n * m, 0.0); p.cuu.assign((size_t)T * m * m, 0.0);
  std::vector<double> J((size_t)rows * w);
  for (int t = 0; t < T; t++) {
    for (double& v : J) v = Uniform();
    for (int i = 0; i < w; i++)
      for (int j = 0; j < w; j++) {
        double s = 0.0;
        for (int r = 0; r < rows; r++) s += J[(size_t)r * w + i] * J[(size_t)r * w + j];
        s /= rows;
        if (i < n && j < n) p.cxx[((size_t)t * n + i) * n + j] = s;
        else if (i < n) p.cxu[((size_t)t * n + i) * m + (j - n)] = s;
        else if (j >= n) p.cuu[((size_t)t * m + (i - n)) * m + (j - n)] = s;
      }
  }
  p.actions.resize((size_t)T * m);
  for (double& v : p.actions) v = 0.5 * Uniform();
  p.limits.resize(2 * (size_t)m);
  for (int i = 0; i < m; i++) { p.limits[2 * i] = -0.6; p.limits[2 * i + 1] = 0.6; }
  return p;
}
bool Finite(const std::vector<double>& v, size_t n) {
  for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
  return true;
}
int Fail(const char* what) { std::printf("riccati FAILED: %s\n", what); return 1; }
}  // namespace

int main() {
  using namespace mjpc_hip;
  {   // box-QP: 21 dimensions, mixed set
    const int n = 21;
    std::vector<double> H((size_t)n * n), M((size_t)n * n), g(n), lo(n), hi(n), res(n, 0.0), R((size_t)n * n, 0.0);
    std::vector<int> index(n, 0);
    for (double& v : M) v = Uniform();
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        double s = i == j ? (double)n : 0.0;
        for (int k = 0; k < n; k++) s += M[(size_t)i * n + k] * M[(size_t)j * n + k];
        H[(size_t)i * n + j] = s;
      }
    for (int i = 0; i < n; i++) { g[i] = 3.0 * n * Uniform(); lo[i] = -0.2 - 0.4 * (Uniform() + 1.0); hi[i] = 0.2 + 0.4 * (Uniform() + 1.0); }
    const int nf = BoxQPSolve(res.data(), R.data(), index.data(), H.data(), g.data(), n, lo.data(), hi.data());
    if (nf < 0 || nf > n) return Fail("box-QP free count");
    for (int i = 0; i < n; i++) if (!(res[i] >= lo[i] && res[i] <= hi[i])) return Fail("box-QP solution outside the box");
    const int again = BoxQPSolve(res.data(), R.data(), index.data(), H.data(), g.data(), n, nullptr, nullptr);      // unbounded: all free
    if (again != n) return Fail("unbounded box-QP");
    for (int i = 0; i < n; i++) H[(size_t)i * n + i] = -1.0;
    std::fill(res.begin(), res.end(), 0.0);
    if (BoxQPSolve(res.data(), R.data(), index.data(), H.data(), g.data(), n, lo.data(), hi.data()) != -1) return Fail("indefinite box-QP");
  }
  for (int limits = 0; limits < 2; limits++) {       // the humanoid's dimensions, both host entry points
    const Problem p = Random(54, 21, 4);
    iLQGSettings s;
    s.action_limits = limits;
    for (int type = 0; type < 4; type++) {
      s.regularization_type = type;
      iLQGBackwardPass bp;
      bp.Allocate(p.n, p.m, p.T);
      BoxQP qp;
      qp.Allocate(p.m);
      std::vector<double> k((size_t)p.T * p.m, 0.0), K((size_t)p.T * p.m * p.n, 0.0);
      int status[3] = {-7, -7, -7};
      bp.RiccatiRegularized(k.data(), K.data(), p.A.data(), p.B.data(), p.cx.data(), p.cu.data(), p.cxx.data(), p.cxu.data(), p.cuu.data(), p.n, p.m, p.T, qp,
                            p.actions.data(), p.limits.data(), s, status);
      if (status[0] != 1 || status[1] != -1 || status[2] != 0) return Fail("status of a regular pass");
      if (!Finite(k, k.size()) || !Finite(K, K.size()) || !Finite(bp.Vxx, (size_t)p.T * p.n * p.n)) return Fail("non-finite output");
      if (limits)
        for (int t = 0; t < p.T - 1; t++)
          for (int i = 0; i < p.m; i++) {
            const double u = p.actions[(size_t)t * p.m + i] + k[(size_t)t * p.m + i];
            if (u < -0.6 - 1e-12 || u > 0.6 + 1e-12) return Fail("control outside its limits");
          }
      // the reference's signature over derivative objects
      ModelDerivatives md;
      CostDerivatives cd;
      md.A = p.A; md.B = p.B; cd.cx = p.cx; cd.cu = p.cu; cd.cxx = p.cxx; cd.cxu = p.cxu; cd.cuu = p.cuu;
      iLQGPolicy policy;
      policy.nu = p.m;
      policy.action_improvement.assign((size_t)p.T * p.m, 0.0); policy.feedback_gain.assign((size_t)p.T * p.m * p.n, 0.0);
      iLQGBackwardPass bp2;
      bp2.Allocate(p.n, p.m, p.T);
      qp.Allocate(p.m);
      if (bp2.Riccati(&policy, &md, &cd, p.n, p.m, p.T, 1.0, qp, p.actions.data(), p.limits.data(), s) != 0) return Fail("Riccati status");
      for (size_t i = 0; i < K.size(); i++) if (policy.feedback_gain[i] != K[i]) return Fail("Riccati and RiccatiRegularized disagree");
    }
  }
  {   // the failing knot: cuu = -10 I and B = 0 at knot 2; regularisation 1, 2, 8 fail there, 64 passes
    Problem p = Random(4, 2, 6);
    const int knot = 2;
    for (int i = 0; i < p.m; i++)
      for (int j = 0; j < p.m; j++) p.cuu[((size_t)knot * p.m + i) * p.m + j] = i == j ? -10.0 : 0.0;
    for (int i = 0; i < p.n * p.m; i++) { p.cxu[(size_t)knot * p.n * p.m + i] = 0.0; p.B[(size_t)knot * p.n * p.m + i] = 0.0; }
    for (int limits = 0; limits < 2; limits++) {
      iLQGSettings s;
      s.action_limits = limits;
      iLQGBackwardPass bp;
      bp.Allocate(p.n, p.m, p.T);
      BoxQP qp;
      qp.Allocate(p.m);
      std::vector<double> k((size_t)p.T * p.m, 0.0), K((size_t)p.T * p.m * p.n, 0.0);
      int status[3] = {0, 0, 0};
      bp.RiccatiRegularized(k.data(), K.data(), p.A.data(), p.B.data(), p.cx.data(), p.cu.data(), p.cxx.data(), p.cxu.data(), p.cuu.data(), p.n, p.m, p.T, qp,
                            p.actions.data(), p.limits.data(), s, status);
      if (status[0] != 1 || status[1] != -1 || status[2] != 3 || bp.regularization != 64.0 || bp.regularization_rate != 8.0) return Fail("regularisation loop");
      s.max_regularization_iterations = 2;
      bp.Reset(p.n, p.m, p.T);
      bp.RiccatiRegularized(k.data(), K.data(), p.A.data(), p.B.data(), p.cx.data(), p.cu.data(), p.cxx.data(), p.cxu.data(), p.cuu.data(), p.n, p.m, p.T, qp,
                            p.actions.data(), p.limits.data(), s, status);
      if (status[0] != 0 || status[1] != knot || status[2] != 2) return Fail("exhausted regularisation loop");
    }
  }
  std::printf("riccati ok\n");
  return 0;
}
