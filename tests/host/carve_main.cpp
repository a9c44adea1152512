// Host test of csrc/carve.h (tests/test_carve.py compiles and runs it, once plain and once under the address / undefined-behaviour
// sanitizers): every layout of the engine's one-step calls, at a handful of shapes, is laid on a null base and on a heap block of
// exactly the reported size.  Fields must be in order, disjoint, aligned to their type and inside the total; both passes must agree;
// every field's full extent is written (the sanitizer sees a write past the block); and every offset and total must equal the closed
// forms the entry points of engine.hip used before the layouts existed, restated here on their own.
// Exit status 0 and "carve ok" when every property holds, otherwise the failed checks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "carve.h"

static int failures = 0;
static long checks = 0;
static void fail(const char *lay, const char *what, const char *field, size_t got, size_t want) {
  if (failures++ < 40) printf("%s: %s %s: got %zu, want %zu\n", lay, field, what, got, want);
}

// one field of a placed layout: where it is, what it holds, and the byte offset from the block's base it had when hand-carved
struct Field { const char *name; const void *p; const void *p_null; size_t elem, n, want; };
#define FD_(l, f, n, w) Field{#f, (l).f, (nul).f, sizeof(*(l).f), (size_t)(n), (size_t)(w)}

static const size_t D = sizeof(double), I = sizeof(int);

// the checks every layout gets.  base / total: the placed pass's block; total_null: what the null pass reported; want_total: closed form
static void check(const char *lay, char *base, size_t total, size_t total_null, size_t want_total, const std::vector<Field> &fields) {
  checks++;
  if (total != total_null) fail(lay, "total of placed and null pass", "", total, total_null);
  if (total != want_total) fail(lay, "total", "", total, want_total);
  size_t end = 0;
  for (const Field &f : fields) {
    if (f.p_null) fail(lay, "null pass gave a pointer", f.name, 1, 0);
    if (!f.p) {                                   // a field the shape switches off: nothing to place
      if (f.n) fail(lay, "null field with elements", f.name, f.n, 0);
      continue;
    }
    const size_t off = (size_t)((const char *)f.p - base);
    if (off != f.want) fail(lay, "offset", f.name, off, f.want);
    if (off < end) fail(lay, "overlaps the field before it", f.name, off, end);
    if (((uintptr_t)f.p) % f.elem) fail(lay, "misaligned", f.name, off, f.elem);
    if (off + f.n * f.elem > total) fail(lay, "ends past the total", f.name, off + f.n * f.elem, total);
    else memset((void *)f.p, 0xA5, f.n * f.elem);
    end = off + f.n * f.elem;
  }
}

// lay() on a null base, then on a heap block of exactly the bytes it reported
#define TWO_PASSES(T, ...)                          \
  T nul, l;                                         \
  Carve c0;                                         \
  lay(c0, nul, __VA_ARGS__);                        \
  char *base = (char *)malloc(c0.bytes() ? c0.bytes() : 1); \
  Carve c1(base);                                   \
  lay(c1, l, __VA_ARGS__);                          \
  const size_t total = c1.bytes(), total_null = c0.bytes()

// ---- closed forms of the hand-carved blocks (doubles unless said otherwise)
static size_t fd_E(const Dims &d, int centered) { return centered ? 1 + 2 * (d.nd + d.nu) : 1 + d.nd + d.nu; }
static size_t fd_doubles(const Dims &d, size_t Tg, int centered) {          // nd_ of fd_pass, spare included
  const size_t R = Tg * fd_E(d, centered), per_t = d.ds + d.nu + 1 + d.nd * d.nd + d.nd * d.nu + d.nr * d.nd + d.nr * d.nu;
  return R * (2 * d.ds + d.nu + 1 + d.nr) + Tg * per_t + 8;
}
static size_t rc_out_doubles(size_t T, size_t n, size_t m) { return T * (m + m * n + n + n * n) + (T - 1) * (n + m + n * n + n * m + m * m) + 6; }
static size_t rc_work(size_t n, size_t m) {                                   // the kernel's work image when it is not in LDS (160 KiB)
  const size_t w = 3 * n * n + 4 * n * m + 3 * m * m + 2 * n + 11 * m + 4;
  return w * D <= 160 * 1024 ? 0 : w;
}

// the pass's own fields: its doubles, and its int tail behind `extra` doubles of the caller's
static void fd_fields(std::vector<Field> &v, const FdLay &l, const FdLay &nul, const Dims &d, size_t Tg, int centered) {
  const size_t R = Tg * fd_E(d, centered), ds = d.ds, nu = d.nu, nr = d.nr, nd = d.nd;
  const size_t ct = R * ds, tt = ct + R * nu, ns = tt + R, rs = ns + R * ds, dx = rs + R * nr, du = dx + Tg * ds, dt = du + Tg * nu, dA = dt + Tg,
               dB = dA + Tg * nd * nd, dC = dB + Tg * nd * nu, dD = dC + Tg * nr * nd;
  v.insert(v.end(), {FD_(l, t.state, R * ds, 0), FD_(l, t.ctrl, R * nu, ct * D), FD_(l, t.time, R, tt * D), FD_(l, t.next, R * ds, ns * D),
                     FD_(l, t.residual, R * nr, rs * D), FD_(l, x, Tg * ds, dx * D), FD_(l, u, Tg * nu, du * D), FD_(l, time, Tg, dt * D),
                     FD_(l, A, Tg * nd * nd, dA * D), FD_(l, B, Tg * nd * nu, dB * D), FD_(l, C, Tg * nr * nd, dC * D), FD_(l, D, Tg * nr * nu, dD * D)});
}
static void fd_int_fields(std::vector<Field> &v, const FdLay &l, const FdLay &nul, const Dims &d, size_t Tg, int centered, size_t extra) {
  const size_t R = Tg * fd_E(d, centered), fl = (fd_doubles(d, Tg, centered) + extra) * D;
  v.insert(v.end(), {FD_(l, t.fail, R, fl), FD_(l, failure, Tg, fl + R * I), FD_(l, dofmap, 2 * d.nv + 2, fl + (R + Tg) * I)});
}
static size_t fd_total(const Dims &d, size_t Tg, int centered, size_t extra) {
  return (fd_doubles(d, Tg, centered) + extra) * D + (Tg * fd_E(d, centered) + Tg + 2 * d.nv + 2) * I;
}

static void test_step(const Dims &d, size_t R) {
  TWO_PASSES(StepTab, d, R);
  const size_t ct = R * d.ds, tt = ct + R * d.nu, ns = tt + R, rs = ns + R * d.ds, nd_ = R * (2 * d.ds + d.nu + 1 + d.nr) + 8;
  check("StepTab", base, total, total_null, nd_ * D + R * I,
        {FD_(l, state, R * d.ds, 0), FD_(l, ctrl, R * d.nu, ct * D), FD_(l, time, R, tt * D), FD_(l, next, R * d.ds, ns * D),
         FD_(l, residual, R * d.nr, rs * D), FD_(l, fail, R, nd_ * D)});
  free(base);
}

static void test_fd(const Dims &d, size_t Tg, int centered) {
  TWO_PASSES(FdLay, d, Tg, centered);
  std::vector<Field> v;
  fd_fields(v, l, nul, d, Tg, centered);
  fd_int_fields(v, l, nul, d, Tg, centered, 0);
  if (l.R != Tg * fd_E(d, centered) || fd_rows_per_knot(d, centered) != fd_E(d, centered)) fail("FdLay", "rows", "R", l.R, Tg * fd_E(d, centered));
  check("FdLay", base, total, total_null, fd_total(d, Tg, centered, 0), v);
  free(base);
}

static void test_cd(const Dims &d, size_t T, int hessians) {
  TWO_PASSES(CdLay, d, T, hessians);
  const size_t nr = d.nr, nd = d.nd, nu = d.nu;
  const size_t n_in = T * (nr + nr * nd + nr * nu), n_g = T * (nr + nd + nu), n_h = hessians ? T * (nd * nd + nu * nu + nd * nu) : 0;
  const size_t dC = T * nr, dD = dC + T * nr * nd, o = dD + T * nr * nu, cx = o + T * nr, cu = cx + T * nd, cxx = cu + T * nu, cuu = cxx + T * nd * nd,
               cxu = cuu + T * nu * nu;
  if (!hessians && (l.out.cxx || l.out.cuu || l.out.cxu)) fail("CdLay", "Hessian fields without Hessians", "cxx", 1, 0);
  if (hessians && !(l.out.cxx && l.out.cuu && l.out.cxu)) fail("CdLay", "no Hessian fields with Hessians", "cxx", 0, 1);
  const size_t h = hessians ? 1 : 0;
  check("CdLay", base, total, total_null, (n_in + n_g + n_h + 8) * D,
        {FD_(l, residual, T * nr, 0), FD_(l, C, T * nr * nd, dC * D), FD_(l, D, T * nr * nu, dD * D), FD_(l, out.cr, T * nr, o * D),
         FD_(l, out.cx, T * nd, cx * D), FD_(l, out.cu, T * nu, cu * D), FD_(l, out.cxx, h * T * nd * nd, cxx * D),
         FD_(l, out.cuu, h * T * nu * nu, cuu * D), FD_(l, out.cxu, h * T * nd * nu, cxu * D)});
  free(base);
}

// the gradient's return block from byte `at` on
static void grad_out_fields(std::vector<Field> &v, const GradOut &l, const GradOut &nul, const Dims &d, size_t T, size_t at) {
  const size_t nu = d.nu, nd = d.nd, Vx = T * nu, Qx = Vx + T * nd, Qu = Qx + (T - 1) * nd, dV = Qu + (T - 1) * nu, n_out = dV + 2;
  v.insert(v.end(), {FD_(l, k, T * nu, at), FD_(l, Vx, T * nd, at + Vx * D), FD_(l, Qx, (T - 1) * nd, at + Qx * D), FD_(l, Qu, (T - 1) * nu, at + Qu * D),
                     FD_(l, dV, 2, at + dV * D), FD_(l, failure, T, at + n_out * D), FD_(l, end, 0, at + (n_out + (T + 1) / 2) * D)});
}
static void test_grad(const Dims &d, size_t T, int centered) {
  const size_t nu = d.nu, nd = d.nd, nr = d.nr;
  const size_t n_out = T * nu + T * nd + (T - 1) * nd + (T - 1) * nu + 2, n_fail = (T + 1) / 2, extra = T * (2 * nr + nd + nu) + n_out + n_fail;
  {
    TWO_PASSES(GradLay, d, T, centered);
    const size_t x0 = fd_doubles(d, T, centered), dcr = x0 + T * nr, dcx = dcr + T * nr, dcu = dcx + T * nd, ob = dcu + T * nu;
    std::vector<Field> v;
    fd_fields(v, l.fd, nul.fd, d, T, centered);
    v.insert(v.end(), {FD_(l, residual, T * nr, x0 * D), FD_(l, cd.cr, T * nr, dcr * D), FD_(l, cd.cx, T * nd, dcx * D), FD_(l, cd.cu, T * nu, dcu * D)});
    if (l.cd.cxx || l.cd.cuu || l.cd.cxu) fail("GradLay", "Hessian fields", "cd.cxx", 1, 0);
    grad_out_fields(v, l.out, nul.out, d, T, ob * D);
    fd_int_fields(v, l.fd, nul.fd, d, T, centered, extra);
    check("GradLay", base, total, total_null, fd_total(d, T, centered, extra), v);
    free(base);
  }
  {
    TWO_PASSES(GradOut, d, T);                    // the pinned mirror
    std::vector<Field> v;
    grad_out_fields(v, l, nul, d, T, 0);
    check("GradOut", base, total, total_null, (n_out + n_fail) * D, v);
    free(base);
  }
}

// the Riccati return block from byte `at` on, with nfail failure ints behind it
static void rc_out_fields(std::vector<Field> &v, const RcOut &l, const RcOut &nul, size_t T, size_t n, size_t m, size_t nfail, size_t at) {
  const size_t K = T * m, Vx = K + T * m * n, Vxx = Vx + T * n, Qx = Vxx + T * n * n, Qu = Qx + (T - 1) * n, Qxx = Qu + (T - 1) * m, Qxu = Qxx + (T - 1) * n * n,
               Quu = Qxu + (T - 1) * n * m, dV = Quu + (T - 1) * m * m, reg = dV + 2, status = reg + 2, n_out = rc_out_doubles(T, n, m);
  v.insert(v.end(), {FD_(l, k, T * m, at), FD_(l, K, T * m * n, at + K * D), FD_(l, Vx, T * n, at + Vx * D), FD_(l, Vxx, T * n * n, at + Vxx * D),
                     FD_(l, Qx, (T - 1) * n, at + Qx * D), FD_(l, Qu, (T - 1) * m, at + Qu * D), FD_(l, Qxx, (T - 1) * n * n, at + Qxx * D),
                     FD_(l, Qxu, (T - 1) * n * m, at + Qxu * D), FD_(l, Quu, (T - 1) * m * m, at + Quu * D), FD_(l, dV, 2, at + dV * D),
                     FD_(l, reg, 2, at + reg * D), FD_(l, status, 3, at + status * D), FD_(l, tail, 0, at + n_out * D),
                     FD_(l, failure, nfail, at + n_out * D), FD_(l, end, 0, at + (n_out + (nfail + 1) / 2) * D)});
}
static void test_rc(size_t T, size_t n, size_t m, int limits) {
  const size_t work = rc_work(n, m), n_out = rc_out_doubles(T, n, m);
  {
    TWO_PASSES(RcLay, T, n, m, limits, work);
    const size_t nn = n * n, nm = n * m, mm = m * m;
    const size_t cnt[9] = {(T - 1) * nn, (T - 1) * nm, T * n, (T - 1) * m, T * nn, (T - 1) * nm, (T - 1) * mm, limits ? (T - 1) * m : 0, limits ? 2 * m : 0};
    size_t at[10] = {0};
    for (int i = 0; i < 9; i++) at[i + 1] = at[i] + cnt[i];
    std::vector<Field> v = {FD_(l, A, cnt[0], at[0] * D), FD_(l, B, cnt[1], at[1] * D), FD_(l, cx, cnt[2], at[2] * D), FD_(l, cu, cnt[3], at[3] * D),
                            FD_(l, cxx, cnt[4], at[4] * D), FD_(l, cxu, cnt[5], at[5] * D), FD_(l, cuu, cnt[6], at[6] * D),
                            FD_(l, actions, cnt[7], at[7] * D), FD_(l, limits, cnt[8], at[8] * D)};
    rc_out_fields(v, l.out, nul.out, T, n, m, 0, at[9] * D);
    v.push_back(FD_(l, scratch, work, (at[9] + n_out) * D));
    check("RcLay", base, total, total_null, (at[9] + n_out + work + 8) * D, v);
    free(base);
  }
  for (size_t nfail : {(size_t)0, T}) {           // the pinned mirror of the backward pass alone and of the whole iteration
    TWO_PASSES(RcOut, T, n, m, nfail);
    std::vector<Field> v;
    rc_out_fields(v, l, nul, T, n, m, nfail, 0);
    check("RcOut", base, total, total_null, (n_out + (nfail + 1) / 2) * D, v);
    free(base);
  }
}

static void test_ilqg(const Dims &d, size_t T, int centered, size_t work) {
  TWO_PASSES(IlqgLay, d, T, centered, work);
  const size_t nu = d.nu, nd = d.nd, nr = d.nr, n_out = rc_out_doubles(T, nd, nu), n_fail = (T + 1) / 2;
  const size_t n_cd = T * (2 * nr + nd + nu + nd * nd + nu * nu + nd * nu), extra = n_cd + 2 * nu + n_out + n_fail + work;
  const size_t x0 = fd_doubles(d, T, centered), cr = x0 + T * nr, cx = cr + T * nr, cu = cx + T * nd, cxx = cu + T * nu, cuu = cxx + T * nd * nd,
               cxu = cuu + T * nu * nu, dlim = x0 + n_cd, ob = dlim + 2 * nu;
  std::vector<Field> v;
  fd_fields(v, l.fd, nul.fd, d, T, centered);
  v.insert(v.end(), {FD_(l, residual, T * nr, x0 * D), FD_(l, cd.cr, T * nr, cr * D), FD_(l, cd.cx, T * nd, cx * D), FD_(l, cd.cu, T * nu, cu * D),
                     FD_(l, cd.cxx, T * nd * nd, cxx * D), FD_(l, cd.cuu, T * nu * nu, cuu * D), FD_(l, cd.cxu, T * nd * nu, cxu * D),
                     FD_(l, limits, 2 * nu, dlim * D)});
  rc_out_fields(v, l.out, nul.out, T, nd, nu, T, ob * D);
  v.push_back(FD_(l, scratch, work, (ob + n_out + n_fail) * D));
  fd_int_fields(v, l.fd, nul.fd, d, T, centered, extra);
  check("IlqgLay", base, total, total_null, fd_total(d, T, centered, extra), v);
  free(base);
}

static void ukf_in_fields(std::vector<Field> &v, const UkfIn &l, const UkfIn &nul, const Dims &d, size_t ns) {
  const size_t L = d.ds, u = L + d.nd * d.nd, np = u + d.nu, nsn = np + d.nd, map = nsn + ns;
  v.insert(v.end(), {FD_(l, x, d.ds, 0), FD_(l, L, d.nd * d.nd, L * D), FD_(l, u, d.nu, u * D), FD_(l, noise_process, d.nd, np * D),
                     FD_(l, noise_sensor, ns, nsn * D), FD_(l, dofmap, 2 * d.nv + 2, map * D), FD_(l, qmap, 2 * d.nq + 2, map * D + (2 * d.nv + 2) * I)});
}
static void ukf_back_fields(std::vector<Field> &v, const UkfBack &l, const UkfBack &nul, const Dims &d, size_t ns, size_t at) {
  const size_t R = 2 * d.nd + 1, mom = R * d.ds, sm = mom + d.ds, ss = sm + ns, sy = ss + d.nd * d.nd, yy = sy + d.nd * ns, fl = yy + ns * ns;
  v.insert(v.end(), {FD_(l, next, R * d.ds, at), FD_(l, state_mean, d.ds, at + mom * D), FD_(l, sensor_mean, ns, at + sm * D),
                     FD_(l, cov_ss, d.nd * d.nd, at + ss * D), FD_(l, cov_sy, d.nd * ns, at + sy * D), FD_(l, cov_yy, ns * ns, at + yy * D),
                     FD_(l, failure, 1, at + fl * D), FD_(l, end, 0, at + (fl + 1) * D)});
}
static void test_ukf(const Dims &d, size_t ns) {
  const size_t ds = d.ds, nu = d.nu, nr = d.nr, nd = d.nd, R = 2 * nd + 1;
  const size_t n_map = 2 * d.nv + 2 + 2 * d.nq + 2, n_in = ds + nd * nd + nu + nd + ns + (n_map + 1) / 2;
  const size_t n_mom = ds + ns + nd * nd + nd * ns + ns * ns + 1, n_back = R * ds + n_mom;
  const size_t n_tab = R * (ds + nu + 1) + R * nr + R * (nd + ns) + (R + 1) / 2;
  {
    TWO_PASSES(UkfLay, d, ns);
    const size_t st = n_in, ct = st + R * ds, tt = ct + R * nu, rs = tt + R, df = rs + R * nr, fl = df + R * (nd + ns);
    std::vector<Field> v;
    ukf_in_fields(v, l.in, nul.in, d, ns);
    v.insert(v.end(), {FD_(l, t.state, R * ds, st * D), FD_(l, t.ctrl, R * nu, ct * D), FD_(l, t.time, R, tt * D), FD_(l, t.residual, R * nr, rs * D),
                       FD_(l, diff, R * (nd + ns), df * D), FD_(l, t.fail, R, fl * D)});
    ukf_back_fields(v, l.back, nul.back, d, ns, (n_in + n_tab) * D);
    if (l.t.next != l.back.next) fail("UkfLay", "next-state rows are not the block's", "t.next", 0, 1);
    check("UkfLay", base, total, total_null, (n_in + n_tab + n_back + 8) * D, v);
    free(base);
  }
  {
    TWO_PASSES(UkfHost, d, ns);
    std::vector<Field> v;
    ukf_in_fields(v, l.in, nul.in, d, ns);
    ukf_back_fields(v, l.back, nul.back, d, ns, n_in * D);
    check("UkfHost", base, total, total_null, (n_in + n_back) * D, v);
    free(base);
  }
}

static void test_fb(const Dims &d, size_t T, size_t H, size_t nl, bool timed) {
  TWO_PASSES(FbLay, d, T, H, nl, timed);
  const size_t ds = d.ds, nu = d.nu, nd = d.nd, row = ds + 2 * nu + nu * nd, h = timed ? 1 : 0;
  const size_t states = T, actions = states + T * ds, impr = actions + T * nu, gain = impr + T * nu, alpha = gain + T * nu * nd, scale = alpha + nl, tab = scale + nl;
  const size_t ubar = tab + H * ds, kbar = ubar + H * nu, Kbar = kbar + H * nu;
  if (!timed && (l.xbar || l.ubar || l.kbar || l.Kbar)) fail("FbLay", "tables in indexed mode", "xbar", 1, 0);
  if (timed && !(l.xbar && l.ubar && l.kbar && l.Kbar)) fail("FbLay", "no tables in time mode", "xbar", 0, 1);
  check("FbLay", base, total, total_null, (T * (row + 1) + 2 * nl + (timed ? H * row : 0) + 8) * D,
        {FD_(l, times, T, 0), FD_(l, states, T * ds, states * D), FD_(l, actions, T * nu, actions * D), FD_(l, improvement, T * nu, impr * D),
         FD_(l, gain, T * nu * nd, gain * D), FD_(l, alpha, nl, alpha * D), FD_(l, scale, nl, scale * D), FD_(l, xbar, h * H * ds, tab * D),
         FD_(l, ubar, h * H * nu, ubar * D), FD_(l, kbar, h * H * nu, kbar * D), FD_(l, Kbar, h * H * nu * nd, Kbar * D)});
  free(base);
}

static Dims dims(size_t nq, size_t nv, size_t na, size_t nu, size_t nr) { return Dims{nq, nv, na, nu, nr, nq + nv + na, 2 * nv + na}; }

int main() {
  // the carver itself: null base, alignment after ints, running total
  {
    Carve c;
    if (c.take<double>(3) || c.take<int>(5) || c.bytes() != 44) fail("Carve", "null base", "", c.bytes(), 44);
    if (c.take<double>(1) || c.bytes() != 56) fail("Carve", "a double behind five ints starts on a whole double", "", c.bytes(), 56);
    alignas(8) char block[64];
    Carve p(block);
    int *i = p.take<int>(1);
    double *x = p.take<double>(2);
    int *j = p.take<int>(0);
    p.align_to<double>();
    if ((char *)i != block || (char *)x != block + 8 || (char *)j != block + 24 || p.bytes() != 24) fail("Carve", "placed", "", p.bytes(), 24);
  }
  // particle-like | no actuator | no residual row | a free joint, mocap-free, odd nd (R = 2 nd + 1 and the int tails odd and even) | activations
  const Dims shapes[] = {dims(2, 2, 0, 2, 3), dims(3, 3, 0, 0, 2), dims(1, 1, 0, 1, 0), dims(19, 18, 1, 12, 37), dims(8, 7, 2, 3, 5), dims(4, 4, 0, 1, 4)};
  for (const Dims &d : shapes) {
    for (size_t R : {1, 2, 5, 40}) test_step(d, R);
    for (int centered = 0; centered < 2; centered++) {
      for (size_t Tg : {1, 2, 3, 6}) test_fd(d, Tg, centered);
      for (size_t T : {2, 3, 6}) {
        test_grad(d, T, centered);
        // the iteration's Riccati scratch in LDS (no work doubles), and outside it (what a model of this size would never need: the layout
        // does not know, it takes the count it is given)
        if (d.nu) for (size_t work : {(size_t)0, rc_work(80, 10)}) test_ilqg(d, T, centered, work);
      }
    }
    for (size_t T : {1, 2, 3, 6}) for (int hessians = 0; hessians < 2; hessians++) test_cd(d, T, hessians);
    for (size_t ns = 1; ns <= d.nr && ns <= 3; ns++) test_ukf(d, ns);
    if (d.nr > 3) test_ukf(d, d.nr);
    if (d.nu) {
      for (size_t T : {2, 3, 6}) for (size_t nl : {1, 3, 8}) { test_fb(d, T, 2, nl, false); test_fb(d, T, 5, nl, true); test_fb(d, T, T, nl, true); }
    }
  }
  // the backward pass takes its own dimensions: small, odd, and one whose work image (3 n^2 + 4 n m + ...) is beyond the LDS limit
  if (rc_work(4, 2) != 0 || rc_work(80, 10) == 0) fail("rc_work", "LDS threshold", "", rc_work(80, 10), 22974);
  for (size_t T : {2, 3, 6}) for (int limits = 0; limits < 2; limits++) { test_rc(T, 4, 2, limits); test_rc(T, 1, 1, limits); test_rc(T, 37, 12, limits); test_rc(T, 80, 10, limits); }
  if (!failures) printf("carve ok (%ld layouts checked)\n", checks);
  return failures ? 1 : 0;
}
