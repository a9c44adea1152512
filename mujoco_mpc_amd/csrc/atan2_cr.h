// atan2_cr.h — atan2(y, x) for y >= 0 rounded from a double-double evaluation (relative error below 2^-100 before the final rounding): the
// same bits on the device, in the 1-lane emulation and on any host, whatever libm stands behind atan2 there.  The feedback head's quaternion
// tangent (feedback.h) must equal the host's StateDiff bit for bit, and atan2 is the one operation of it that IEEE 754 does not pin: the
// device library's result is a last place off the host's now and then.  The result here is the correctly rounded one
// unless the exact value lies within 2^-100 (relative) of a rounding boundary; tests/golden/atan2_cr.json holds 2208 checked arguments.
// Method: t = min(y, |x|) / max(y, |x|) in double-double; c = round(32 t) / 32; atan t = atan c (table) + atan u, u = (t - c) / (1 + t c),
// |u| <= 2^-6, by twelve terms of the series in u^2; pi/2 - atan t when y > |x|; pi - that when x < 0.  Every operation is spelled with an
// explicit error term (fma for the products) and nothing is contracted, so the evaluation does not depend on compiler flags.  The host's
// StateDiff (planner.cc) calls the same function: device and host agree by construction.  glibc's atan2 differs from it in about 3 of
// 10^4 arguments (its error reaches 0.5003 ulp there; checked against 300-bit arithmetic), the device library's far more often.  Zero,
// non-finite and arguments beyond 1e-150 .. 1e150 go to the library's atan2 (zero: the value is exact).
#pragma once
#include <math.h>
// stands alone: the device and emulation builds reach it through core.h (DEV is theirs), the host planner includes it directly
#ifdef DEV
#define DD_FN DEV
#else
#define DD_FN static inline
#endif
#ifdef __clang__
#define DD_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define DD_NOCONTRACT          /* built with -ffp-contract=off */
#endif

struct DD { double hi, lo; };
DD_FN DD dd_quick(double a, double b) {
  DD_NOCONTRACT
  DD r; r.hi = a + b; r.lo = b - (r.hi - a); return r;
}
DD_FN DD dd_two_sum(double a, double b) {
  DD_NOCONTRACT
  DD r; r.hi = a + b; const double bb = r.hi - a; r.lo = (a - (r.hi - bb)) + (b - bb); return r;
}
DD_FN DD dd_two_prod(double a, double b) {
  DD_NOCONTRACT
  DD r; r.hi = a * b; r.lo = __builtin_fma(a, b, -r.hi); return r;
}
DD_FN DD dd_add(DD a, DD b) {
  DD_NOCONTRACT
  DD s = dd_two_sum(a.hi, b.hi); const DD t = dd_two_sum(a.lo, b.lo);
  s.lo = s.lo + t.hi; s = dd_quick(s.hi, s.lo);
  s.lo = s.lo + t.lo; return dd_quick(s.hi, s.lo);
}
DD_FN DD dd_neg(DD a) { DD r; r.hi = -a.hi; r.lo = -a.lo; return r; }
DD_FN DD dd_mul(DD a, DD b) {
  DD_NOCONTRACT
  DD p = dd_two_prod(a.hi, b.hi);
  const double c1 = a.hi * b.lo, c2 = a.lo * b.hi;
  p.lo = p.lo + (c1 + c2);
  return dd_quick(p.hi, p.lo);
}
DD_FN DD dd_mul_d(DD a, double b) {
  DD_NOCONTRACT
  DD p = dd_two_prod(a.hi, b);
  p.lo = p.lo + a.lo * b;
  return dd_quick(p.hi, p.lo);
}
DD_FN DD dd_div(DD a, DD b) {
  DD_NOCONTRACT
  const double q1 = a.hi / b.hi;
  DD r = dd_add(a, dd_neg(dd_mul_d(b, q1)));
  const double q2 = r.hi / b.hi;
  r = dd_add(r, dd_neg(dd_mul_d(b, q2)));
  const double q3 = r.hi / b.hi;
  DD q = dd_quick(q1, q2);
  DD e; e.hi = q3; e.lo = 0.0;
  return dd_add(q, e);
}

// atan(k / 32), k = 0 .. 32, and (-1)^k / (2k + 1), k = 0 .. 11, to double-double precision
DD_FN DD atan2_cr_table(int k) {
  static const double T[33][2] = {
    {0x0.0p+0, 0x0.0p+0},
    {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},
    {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},
    {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},
    {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},
    {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},
    {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},
    {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},
    {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
    {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},
    {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},
    {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},
    {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},
    {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},
    {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},
    {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},
    {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},
    {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},
    {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},
    {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},
    {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
    {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},
    {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},
    {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},
    {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},
    {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},
    {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},
    {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},
    {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},
    {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},
    {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},
    {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},
    {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55},
  };
  DD r; r.hi = T[k][0]; r.lo = T[k][1]; return r;
}
DD_FN DD atan2_cr_coef(int k) {
  static const double Cf[12][2] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {-0x1.5555555555555p-2, -0x1.5555555555555p-56},
    {0x1.999999999999ap-3, -0x1.999999999999ap-57},
    {-0x1.2492492492492p-3, -0x1.2492492492492p-57},
    {0x1.c71c71c71c71cp-4, 0x1.c71c71c71c71cp-58},
    {-0x1.745d1745d1746p-4, 0x1.745d1745d1746p-59},
    {0x1.3b13b13b13b14p-4, -0x1.3b13b13b13b14p-58},
    {-0x1.1111111111111p-4, -0x1.1111111111111p-60},
    {0x1.e1e1e1e1e1e1ep-5, 0x1.e1e1e1e1e1e1ep-61},
    {-0x1.af286bca1af28p-5, -0x1.af286bca1af28p-59},
    {0x1.8618618618618p-5, 0x1.8618618618618p-59},
    {-0x1.642c8590b2164p-5, -0x1.642c8590b2164p-60},
  };
  DD r; r.hi = Cf[k][0]; r.lo = Cf[k][1]; return r;
}

DD_FN double atan2_cr(double y, double x) {
  DD_NOCONTRACT
  const double ax = fabs(x);
  const double big = ax > y ? ax : y, small = ax > y ? y : ax;
  if (!(y > 0.0) || !(ax > 0.0) || !(big < 1.0e150) || !(small > 1.0e-150)) return atan2(y, x);
  DD num, den; num.hi = small; num.lo = 0.0; den.hi = big; den.lo = 0.0;
  const DD t = dd_div(num, den);
  const int k = (int)(t.hi * 32.0 + 0.5);
  DD c; c.hi = k * 0.03125; c.lo = 0.0;
  DD one; one.hi = 1.0; one.lo = 0.0;
  const DD u = dd_div(dd_add(t, dd_neg(c)), dd_add(one, dd_mul_d(t, c.hi)));
  const DD u2 = dd_mul(u, u);
  DD p = atan2_cr_coef(11);
  for (int i = 10; i >= 0; i--) p = dd_add(dd_mul(p, u2), atan2_cr_coef(i));
  DD r = dd_add(atan2_cr_table(k), dd_mul(p, u));
  DD half_pi; half_pi.hi = 0x1.921fb54442d18p+0; half_pi.lo = 0x1.1a62633145c07p-54;
  DD pi; pi.hi = 0x1.921fb54442d18p+1; pi.lo = 0x1.1a62633145c07p-53;
  if (y > ax) r = dd_add(half_pi, dd_neg(r));
  if (x < 0.0) r = dd_add(pi, dd_neg(r));
  return r.hi + r.lo;
}
