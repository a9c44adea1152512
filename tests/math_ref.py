"""Exact references, input sets and CPU restatements for the device's scalar maths (csrc/dmath.h) and linear solves
(csrc/linalg.h, csrc/noslip.h).  No GPU here: tests/test_math_ref.py proves this module sound on the CPU tier,
tests/test_gpu_math.py holds the device against it.

Scalar references are mpmath values at 200 bits, handed out as (hi, lo, ulp) triples of doubles: hi + lo is the exact value to
about 106 bits and ulp is the spacing of doubles at the exact value, so an error in ulps is one vectorised expression.
Residuals of linear systems are formed in exact integer arithmetic (every double is an integer times a power of two), which is
stronger than any fixed precision."""
import ctypes
import functools
import os
import subprocess
import tempfile

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.prec = 200
D_MINVAL = 1e-15
U = 2.0 ** -53
N_CLASS = 20000                 # random arguments per class
SEED = 0x4D415448


# ---- exact values as double triples ---------------------------------------------------------------------------------------------
class Exact:
    """exact = hi + lo (to ~2^-106 relative); ulp = spacing of doubles at |exact| (2^-1074 at and below the denormals)"""
    def __init__(self, values):
        n = len(values)
        self.hi, self.lo, self.ulp = np.zeros(n), np.zeros(n), np.zeros(n)
        for i, v in enumerate(values):
            hi = float(v)
            self.hi[i] = hi
            if not np.isfinite(hi):
                self.lo[i], self.ulp[i] = 0.0, np.inf
                continue
            self.lo[i] = float(v - MP.mpf(hi))
            if v == 0:
                self.ulp[i] = 2.0 ** -1074
            else:
                _, e = MP.frexp(v)                    # |v| = m 2^e, 0.5 <= m < 1
                self.ulp[i] = 2.0 ** max(int(e) - 53, -1074)


def ulp_error(got, exact):
    """signed error of the doubles `got` against an Exact, in ulps of the exact value"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((got - exact.hi) - exact.lo) / exact.ulp


def vec_error(got, hi, lo):
    """error of vector results (rows of got against rows of hi + lo) in units of 2^-53 of the exact result's norm"""
    d = (np.asarray(got) - hi) - lo
    nrm = np.sqrt((hi * hi).sum(axis=-1))
    return np.abs(d).max(axis=-1) / (U * nrm)


def _mpf(a):
    return [MP.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def ref_rcp(x): return Exact([1 / v for v in _mpf(x)])
def ref_rsqrt(x): return Exact([1 / MP.sqrt(v) for v in _mpf(x)])
def ref_sqrt(x): return Exact([MP.sqrt(v) for v in _mpf(x)])
def ref_div(a, b): return Exact([p / q for p, q in zip(_mpf(a), _mpf(b))])
def ref_pow(x, p): return Exact([MP.power(v, q) for v, q in zip(_mpf(x), _mpf(p))])
def ref_sincos(x):
    v = _mpf(x)
    return Exact([MP.sin(t) for t in v]), Exact([MP.cos(t) for t in v])


# ---- input sets -----------------------------------------------------------------------------------------------------------------
def _rng(tag):
    return np.random.default_rng([SEED, sum(tag.encode())])


def _random_normals(rng, n, emin, emax):
    return np.ldexp(1.0 + rng.random(n), rng.integers(emin, emax + 1, n).astype(np.int32))


def _neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def _obj(a):
    return np.asarray(a, dtype=np.int64).astype(object)


def near_boundary(kind, rng, ncand=300000):
    """arguments whose exact result lies within 2^-60 (relative) of the midpoint between two doubles: candidates are built from
    random midpoints m = (2 Q + 1) 2^-53 in (1, 2) and kept when the exact integer test passes.  Returns (x, y)."""
    Q = (1 << 52) + rng.integers(0, 1 << 52, ncand, dtype=np.int64)
    M = 2 * _obj(Q) + 1                                              # m = M 2^-53
    ml = np.ldexp(Q.astype(np.longdouble) * 2 + 1, -53)              # 64-bit mantissa: m itself
    if kind == "rcp":                                                # x = 1/m in (0.5, 1): X = x 2^53
        x = (1 / ml).astype(np.float64)
        keep = np.abs(_obj(np.ldexp(x, 53)) * M - (1 << 106)) <= (1 << 46)
        return x[keep.astype(bool)], None
    if kind == "sqrt":                                               # x = m^2 in (1, 4): X = x 2^52
        x = (ml * ml).astype(np.float64)
        M2 = M * M
        keep = np.abs((_obj(np.ldexp(x, 52)) << 54) - M2) <= (M2 >> 60)
        return x[keep.astype(bool)], None
    if kind == "rsqrt":                                              # x = 1/m^2 in (0.25, 1): X = x 2^54
        x = (1 / (ml * ml)).astype(np.float64)
        keep = np.abs(_obj(np.ldexp(x, 54)) * M * M - (1 << 160)) <= (1 << 100)
        return x[keep.astype(bool)], None
    B = (1 << 52) + rng.integers(0, 1 << 52, ncand, dtype=np.int64)  # div: b = B 2^-52 in [1, 2), a = m b in (1, 4): A = a 2^52
    b = np.ldexp(B.astype(np.float64), -52)
    a = (ml * b.astype(np.longdouble)).astype(np.float64)
    MB = M * _obj(B)
    keep = np.abs((_obj(np.ldexp(a, 52)) << 53) - MB) <= (MB >> 60)
    return a[keep.astype(bool)], b[keep.astype(bool)]


@functools.lru_cache(maxsize=None)
def scalar_classes(fn):
    """accuracy classes of fn in ('rcp', 'rsqrt', 'sqrt', 'div'): {class: (x, y)}; y is the divisor of 'div', else None.
    Every argument is a positive normal double whose result is a normal double (the rest is the edge class)."""
    rng = _rng("scalar" + fn)
    k = np.arange(0, 65, dtype=np.float64)
    around_one = np.concatenate([1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -53, 1.0 - k * 2.0 ** -52])
    squares = rng.integers(1 << 20, 1 << 26, 400).astype(np.float64) ** 2
    mu = np.linspace(0.01, 2.0, 200)
    sites = np.concatenate([[1e-15, 1e-10], 10.0 ** np.linspace(-2, 10, 241), mu * mu * (1 + mu * mu)])
    lo_e, hi_e = (-1021, 1021) if fn in ("rcp", "div") else (-1022, 1023)
    pow2 = _neighbours(np.ldexp(1.0, np.arange(lo_e + 1, hi_e, dtype=np.int32)))
    c = {
        "random": _random_normals(rng, N_CLASS, lo_e, hi_e),
        "powers_of_two": pow2,
        "around_one_and_squares": np.concatenate([around_one, _neighbours(squares)]),
        "call_sites": _neighbours(sites),
    }
    xb, yb = near_boundary(fn, rng)
    if fn != "div":
        c["rounding_boundary"] = xb
        return {name: (x, None) for name, x in c.items()}
    out = {}
    for name, x in c.items():
        if name == "random":
            out[name] = (_random_normals(rng, x.size, -500, 500), _random_normals(rng, x.size, -500, 500))
        else:
            out[name] = (rng.permutation(x)[:x.size], x) if name != "powers_of_two" else (_random_normals(rng, x.size, -1, 1), x)
    out["rounding_boundary"] = (xb, yb)
    return out


PIO2 = MP.pi / 2
KMAX = 41                      # |x| < 64: |rint(x 2/pi)| <= 41


def _around(values_mp):
    return _neighbours(np.array([float(v) for v in values_mp]))


@functools.lru_cache(maxsize=None)
def sincos_classes():
    rng = _rng("sincos")
    ks = [k for k in range(-KMAX, KMAX + 1)]
    halves = np.array([float((k + MP.mpf(0.5)) * PIO2) for k in range(-KMAX, KMAX) if abs(float((k + 0.5) * PIO2)) < 63.9])
    steps = np.arange(-8, 9)
    rint_edge = halves[:, None] * (1.0 + steps[None, :] * 2.0 ** -52)            # up to 8 doubles either side
    tiny = 10.0 ** -np.arange(1, 324, dtype=np.float64)
    return {
        "abs_le_20": rng.uniform(-20.0, 20.0, N_CLASS),
        "abs_20_to_64": rng.uniform(20.0, 64.0, N_CLASS) * rng.choice([-1.0, 1.0], N_CLASS),
        "tiny": np.concatenate([tiny, -tiny, [5e-324, -5e-324, 2.2250738585072014e-308]]),
        "k_pio2": _around([k * PIO2 for k in ks if k != 0]),
        "k_half_pio2": _neighbours(halves),
        "rint_decision": rint_edge.ravel(),
        "below_64": np.array([np.nextafter(64.0, 0), -np.nextafter(64.0, 0), 63.999, -63.999]),
    }


SINCOS_LIBM_CLASS = np.array([64.0, -64.0, np.nextafter(64.0, np.inf), -np.nextafter(64.0, np.inf), 100.0, -1e5, 1e15])
# derived absolute term of d_sincos next to the multiples of pi/2: 41 x (truncation of the two-term constant, 3.5e-27, +
# rounding of k * pio2_1t, 2^-53 x 6.1e-11)
SINCOS_ABS = 4.2e-25
# maxima of the two CPU restatements of d_sincos over the classes above against the 200-bit value (ulps of the exact value
# beyond the absolute term), as tests/test_math_ref.py measures and pins them; the device bar is the larger one + 0.5 ulp
SINCOS_CPU_MAX = {"uncontracted": 1.47, "fused": 1.47}       # both 1.4636 at x = 57.33802827302554 (20 < |x| < 64)

EDGE_ARGS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, 1e-310, 5.6e-309,
                      1.7976931348623157e308, -1.7976931348623157e308, -1.0, -1e-300, 2.2250738585072014e-308,
                      np.ldexp(1.0, 1022), np.ldexp(1.5, 1023)])


# ---- CPU restatements of the device sequences -----------------------------------------------------------------------------------
_C_SRC = r"""
#include <math.h>
#define F __builtin_fma
void rsqrt_seq(int n, const double *x, const double *seed, double *o, int steps, int fused) {
  for (int i = 0; i < n; i++) {
    double y = seed[i];
    for (int s = 0; s < steps; s++) { double t = 0.5 * x[i] * y; y = fused ? y * F(-t, y, 1.5) : y * (1.5 - t * y); }
    o[i] = y;
  }
}
static double rcp1(double x, double y, int steps) {
  for (int s = 0; s < steps; s++) { double e = F(-x, y, 1.0); y = F(y, e, y); }
  return y;
}
void rcp_seq(int n, const double *x, const double *seed, double *o, int steps) { for (int i = 0; i < n; i++) o[i] = rcp1(x[i], seed[i], steps); }
void div_seq(int n, const double *a, const double *b, const double *seed, double *o) {
  for (int i = 0; i < n; i++) { double r = rcp1(b[i], seed[i], 2), q = a[i] * r; o[i] = F(r, F(-b[i], q, a[i]), q); }
}
void sqrt_seq(int n, const double *x, const double *seed, double *o, int fused) {
  for (int i = 0; i < n; i++) {
    double y = seed[i];
    for (int s = 0; s < 2; s++) { double t = 0.5 * x[i] * y; y = fused ? y * F(-t, y, 1.5) : y * (1.5 - t * y); }
    double s = x[i] * y; o[i] = F(0.5 * y, F(-s, s, x[i]), s);
  }
}
void sincos_seq(int n, const double *xs, double *sn, double *cs, int fused, int qflip) {
  static const double S[6] = {-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10};
  static const double C[6] = {4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11};
  for (int i = 0; i < n; i++) {
    double x = xs[i], k = rint(x * 0.63661977236758134308), r, z, ps, pc, s, c;
    if (fused) r = F(-k, 6.07710050650619224932e-11, F(-k, 1.57079632673412561417e+00, x));
    else r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    z = r * r;
    if (fused) {
      ps = F(z, F(z, F(z, F(z, F(z, S[5], S[4]), S[3]), S[2]), S[1]), S[0]);
      pc = F(z, F(z, F(z, F(z, F(z, C[5], C[4]), C[3]), C[2]), C[1]), C[0]);
      s = F(r * z, ps, r); c = F(z * z, pc, F(-0.5, z, 1.0));
    } else {
      ps = S[0] + z * (S[1] + z * (S[2] + z * (S[3] + z * (S[4] + z * S[5]))));
      pc = C[0] + z * (C[1] + z * (C[2] + z * (C[3] + z * (C[4] + z * C[5]))));
      s = r + r * z * ps; c = 1.0 - 0.5 * z + z * z * pc;
    }
    int q = (((int)k) & 3) ^ qflip;
    double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    sn[i] = (q & 2) ? -s1 : s1; cs[i] = ((q + 1) & 2) ? -c1 : c1;
  }
}
"""


@functools.lru_cache(maxsize=None)
def _clib():
    """the restated sequences need a true fma, which numpy does not have: a few lines of C, built into a temporary directory"""
    d = tempfile.mkdtemp(prefix="mjpc_math_ref_")
    src, so = os.path.join(d, "seq.c"), os.path.join(d, "seq.so")
    with open(src, "w") as f:
        f.write(_C_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, "-lm"])
    return ctypes.CDLL(so)


def _p(a): return a.ctypes.data_as(ctypes.c_void_p)
def _c(a): return np.ascontiguousarray(a, dtype=np.float64)


def seed_of(exact, delta):
    """the hardware seed modelled as the correctly rounded value times (1 + delta)"""
    return exact.hi * (1.0 + delta)


def seq_rsqrt(x, seed, steps=2, fused=0):
    x, seed, o = _c(x), _c(seed), np.zeros(len(x))
    _clib().rsqrt_seq(len(x), _p(x), _p(seed), _p(o), steps, fused)
    return o


def seq_rcp(x, seed, steps=2):
    x, seed, o = _c(x), _c(seed), np.zeros(len(x))
    _clib().rcp_seq(len(x), _p(x), _p(seed), _p(o), steps)
    return o


def seq_div(a, b, seed):
    a, b, seed, o = _c(a), _c(b), _c(seed), np.zeros(len(a))
    _clib().div_seq(len(a), _p(a), _p(b), _p(seed), _p(o))
    return o


def seq_sqrt(x, seed, fused=0):
    x, seed, o = _c(x), _c(seed), np.zeros(len(x))
    _clib().sqrt_seq(len(x), _p(x), _p(seed), _p(o), fused)
    return o


def seq_sincos(x, fused, qflip=0):
    x = _c(x)
    s, c = np.zeros(len(x)), np.zeros(len(x))
    _clib().sincos_seq(len(x), _p(x), _p(s), _p(c), fused, qflip)
    return s, c


def sincos_excess(got, exact):
    """error beyond the derived absolute term, in ulps of the exact value: (|err| - SINCOS_ABS) / ulp, at least 0"""
    with np.errstate(all="ignore"):
        err = np.abs((got - exact.hi) - exact.lo)
    return np.maximum(err - SINCOS_ABS, 0.0) / exact.ulp


# ---- quaternion references (from the definitions) -------------------------------------------------------------------------------
def _split_rows(rows):
    hi = np.array([[float(v) for v in r] for r in rows])
    lo = np.array([[float(v - MP.mpf(float(v))) for v in r] for r in rows])
    return hi, lo


def _mp_mulquat(a, b):
    return [a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
            a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]]


def _mp_norm(v):
    return MP.sqrt(sum(t * t for t in v))


def _mp_exp(axis, angle):
    """exponential map: unit axis, angle -> (cos(angle/2), axis sin(angle/2))"""
    return [MP.cos(angle / 2)] + [a * MP.sin(angle / 2) for a in axis]


def ref_normalize4(inp):
    rows = []
    for r in inp:
        q = _mpf(r[:4]); n = _mp_norm(q)
        rows.append([t / n for t in q])
    return _split_rows(rows)


def ref_axisangle2quat(inp):
    return _split_rows([_mp_exp(_mpf(r[:3]), MP.mpf(float(r[3]))) for r in inp])


def ref_quatintegrate(inp):
    """q / |q| times the exponential map of scale * vel (axis (1, 0, 0) below D_MINVAL, as the device takes it)"""
    rows = []
    for r in inp:
        q = _mpf(r[:4]); v = _mpf(r[4:7]); h = MP.mpf(float(r[7]))
        nq, nv = _mp_norm(q), _mp_norm(v)
        axis = [t / nv for t in v] if nv >= D_MINVAL else [MP.mpf(1), MP.mpf(0), MP.mpf(0)]
        rows.append(_mp_mulquat([t / nq for t in q], _mp_exp(axis, h * nv)))
    return _split_rows(rows)


def ref_subquat(inp):
    """log map of conj(qb) qa: axis * angle with the angle wrapped into (-pi, pi]"""
    rows = []
    for r in inp:
        qa, qb = _mpf(r[:4]), _mpf(r[4:8])
        qd = _mp_mulquat([qb[0], -qb[1], -qb[2], -qb[3]], qa)
        s = _mp_norm(qd[1:])
        if s == 0:
            rows.append([MP.mpf(0)] * 3); continue
        ang = 2 * MP.atan2(s, qd[0])
        if ang > MP.pi: ang -= 2 * MP.pi
        rows.append([t / s * ang for t in qd[1:]])
    return _split_rows(rows)


def ref_quat2mat(inp):
    rows = []
    for r in inp:
        w, x, y, z = _mpf(r[:4])
        rows.append([w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
                     2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z])
    return _split_rows(rows)


ANGLES = np.array([0.0, 1e-300, 1e-17, 1e-9, 1e-3, 1.0, np.pi - 1e-9, np.pi, 2 * np.pi, 4 * np.pi, 10 * np.pi])
NORM_OFF = np.array([1.0, 1 + 1e-16, 1 - 1e-16, 1 + 1e-15, 1 - 1e-15, 1 + 3e-15, 1 + 1e-8, 1 - 1e-8, 2.0])


def _unit(rng, n, dim, floor=0.05):
    """random unit vectors whose components all exceed `floor` in magnitude (no accidental zeros)"""
    v = rng.uniform(floor * 2, 1.0, (n, dim)) * rng.choice([-1.0, 1.0], (n, dim))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


@functools.lru_cache(maxsize=None)
def quat_inputs(fn):
    """n x 8 input rows of the vector hook for fn (layout at mjpc_hip_math_vector), with a label per row"""
    rng = _rng("quat" + fn)
    rows, labels = [], []
    def add(label, *parts):
        r = np.zeros(8); v = np.concatenate([np.atleast_1d(p) for p in parts]); r[:v.size] = v
        rows.append(r); labels.append(label)
    if fn == "normalize4":
        for off in NORM_OFF:
            for q in _unit(rng, 24, 4): add(f"norm {float(off)!r}", q * off)
    elif fn == "axisangle2quat":
        for ang in np.concatenate([ANGLES, -ANGLES[1:]]):
            for ax in _unit(rng, 16, 3): add(f"angle {float(ang)!r}", ax, ang)
    elif fn == "quatintegrate":
        for ang in ANGLES[:8]:                                  # one step turns a body by at most pi
            for off in NORM_OFF:
                q, ax = _unit(rng, 1, 4)[0] * off, _unit(rng, 1, 3)[0]
                h = 10.0 ** rng.uniform(-3, -1)
                add(f"angle {float(ang)!r} norm {float(off)!r}", q, ax * (ang / h), h)
        for q in _unit(rng, 32, 4): add("below D_MINVAL", q, _unit(rng, 1, 3)[0] * 1e-17, 0.01)
        for q in _unit(rng, 32, 4): add("zero velocity", q, np.zeros(3), 0.01)
    elif fn == "subquat":
        for ang in [1e-300, 1e-17, 1e-9, 1e-3, 1.0, np.pi - 1e-3, -1.0, -1e-9]:
            for _ in range(16):
                qb, ax = _unit(rng, 1, 4)[0], _unit(rng, 1, 3)[0]
                qr = np.concatenate([[np.cos(ang / 2)], ax * np.sin(ang / 2)])
                qa = np.array([float(v) for v in _mp_mulquat(_mpf(qb), _mpf(qr))])
                add(f"angle {ang!r}", qa, qb)
        for q in _unit(rng, 32, 4): add("equal", q, q)
        for q in _unit(rng, 32, 4): add("antipodal", q, -q)
        for eps in [1e-12, 1e-9, 1e-6]:
            for _ in range(16):
                q = _unit(rng, 1, 4)[0]
                p = -q + eps * rng.standard_normal(4)
                add(f"nearly antipodal {eps!r}", q, p / np.sqrt((p * p).sum()))
    elif fn == "quat2mat":
        for q in _unit(rng, 128, 4): add("unit", q)
        for q in _unit(rng, 32, 4): add("scaled", q * 10.0 ** rng.uniform(-3, 3))
    return np.array(rows), labels


# ---- linear systems -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dof_parent(n):
    """the elimination tree of the n-dof model (dof_parentid; the hand's cube joint is the hub above the wrist, csrc/model.h)"""
    from mujoco_mpc_amd.modelgen import humanoid_track, quadruped, shadow_hand
    m = {18: quadruped, 27: humanoid_track, 33: shadow_hand}[n]()[0]
    par = [int(p) for p in m["dof_parentid"]]
    if n == 33:
        par[9] = 8
    return tuple(par)


def chain_parent(n):
    """pattern for the generic solver's sizes: any tree will do, a single chain is the dense pattern"""
    return tuple(range(-1, n - 1))


CONDS = {"1e2": 1e2, "1e6": 1e6, "1e10": 1e10, "1e13": 1e13}


def _chains(par):
    n = len(par)
    leaves = [i for i in range(n) if i not in par]
    out = []
    for leaf in leaves:
        c, a = [], leaf
        while a >= 0:
            c.append(a); a = par[a]
        out.append(np.array(c))
    return out


def make_system(rng, par, cond, tree):
    """A = M + s J^T D J: M = L^T Dm L on the ancestor pattern (unit L, so no fill), J rows on one root-to-leaf chain (tree) or
    across the branches (dense), fewer rows than dofs, D log-uniform over up to ten decades; s is found by bisection so that the
    condition number lands near `cond` (the certified value is computed afterwards, cond_inf).  Symmetric, both triangles filled."""
    n = len(par)
    L = np.eye(n)
    for i in range(n):
        anc, a = [], par[i]
        while a >= 0:
            anc.append(a); a = par[a]
        for a in anc:
            L[i, a] = rng.normal() * 0.3 / len(anc)          # (long chains stay well conditioned: M alone is below the 1e2 class)
    M = L.T @ np.diag(10.0 ** rng.uniform(0, 0.5, n)) @ L
    M = (M + M.T) / 2
    if n == 1:
        return M * cond ** rng.uniform(-0.5, 0.5)
    decades = min(10.0, np.log10(cond))
    chains = _chains(par)
    W = np.zeros((n, n))
    for _ in range(max(1, n // 2)):
        j = np.zeros(n)
        if tree:
            c = chains[rng.integers(len(chains))]
            j[c] = rng.normal(size=c.size)
        else:
            j[:] = rng.normal(size=n)
        W += 10.0 ** -rng.uniform(0, decades) * np.outer(j, j)
    W = (W + W.T) / 2
    lo, hi = -6.0, 20.0
    for _ in range(30):
        mid = (lo + hi) / 2
        if np.linalg.cond(M + 10.0 ** mid * W, np.inf) < cond: lo = mid
        else: hi = mid
    return M + 10.0 ** lo * W


def to_int(a):
    """doubles as exact integers over one common power of two: a = I * 2^e (object array of Python ints, int e)"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64).astype(object)
    e = np.where(a == 0, 0, e.astype(np.int64) - 53)
    emin = int(e[a != 0].min()) if (a != 0).any() else 0
    sh = np.where(a == 0, 0, e - emin).astype(object)
    return mi * (2 ** sh), emin


def exact_residual(A, x, b, x_lo=None):
    """b - A (x + x_lo) exactly (vectors or matrices of columns), rounded once to doubles"""
    Ai, ea = to_int(A); bi, eb = to_int(b)
    parts = [to_int(x)] + ([to_int(x_lo)] if x_lo is not None else [])
    e = min([eb] + [ea + ex for _, ex in parts])
    r = bi * 2 ** (eb - e)
    for xi, ex in parts:
        r = r - Ai.dot(xi) * 2 ** (ea + ex - e)
    return np.ldexp(np.array([float(v) for v in r.ravel()]), e).reshape(r.shape)


def backward_error(A, x, b):
    """normwise backward error eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), the residual exact"""
    r = exact_residual(A, x, b)
    return np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


def exact_solution(A, b, steps=5):
    """x = A^-1 b as hi + lo by iterative refinement on the exact residual (each step gains a factor 1 / (cond * 2^-53))"""
    hi = np.linalg.solve(A, b); lo = np.zeros_like(hi)
    for _ in range(steps):
        d = np.linalg.solve(A, exact_residual(A, hi, b, lo))
        s = hi + (lo + d)
        lo = (hi - s) + (lo + d); hi = s
    return hi, lo


def cond_inf(A):
    """(lower, upper) bounds of |A|_inf |A^-1|_inf certified by the exact residual R = I - A X of an approximate inverse X:
    |X| / (1 + |R|) <= |A^-1| <= |X| / (1 - |R|)"""
    n = A.shape[0]
    X = np.linalg.inv(A)
    for _ in range(2):                                  # one Newton-Schulz step on the exact residual tightens X
        R = exact_residual(A, X, np.eye(n))
        rn = np.abs(R).sum(axis=1).max()
        if rn < 1e-6:
            break
        X = X + X @ R
    assert rn < 0.5, rn
    na, nx = np.abs(A).sum(axis=1).max(), np.abs(X).sum(axis=1).max()
    return na * nx / (1 + rn), na * nx / (1 - rn)


def eta_bar(n):
    """Higham's worst case n * gamma_(3n+1) for a Cholesky-type solve, doubled for a 1-ulp reciprocal"""
    return 2.0 * n * (3 * n + 1) * U


SYSTEMS = 8                     # systems per (size, class, order)


@functools.lru_cache(maxsize=None)
def ldl_systems(n, generic=False):
    """(A (S, n, n), b (S, n), cls (S,), tree (S,), certified cond bounds (S, 2)) for every condition class and order; the last right-hand
    side of each group is aligned with the smallest eigenvector"""
    rng = np.random.default_rng([SEED, n, int(generic)])
    par = chain_parent(n) if generic else dof_parent(n)
    A, b, cls, trees, conds = [], [], [], [], []
    for ci, cond in enumerate(CONDS.values()):
        for tree in ((0,) if generic else (0, 1)):
            for s in range(2 if generic else SYSTEMS):
                a = make_system(rng, par, cond, tree)
                rhs = rng.standard_normal(n)
                if s == 0:
                    rhs = np.linalg.eigh(a)[1][:, 0].copy()
                A.append(a); b.append(rhs); cls.append(ci); trees.append(tree); conds.append(cond_inf(a))
    return np.array(A), np.array(b), np.array(cls), np.array(trees), np.array(conds)


def ldl_numpy(A, b, clamp=D_MINVAL):
    """the bottom-up L^T D L of csrc/linalg.h restated with IEEE divides: pivots from the last dof up, the D_MINVAL clamp on
    every pivot, x = L^-1 D^-1 L^-T b.  Returns (x, smallest pivot before clamping)."""
    a = np.array(A, dtype=np.float64); x = np.array(b, dtype=np.float64); n = len(x)
    Lm = np.zeros((n, n)); rinv = np.zeros(n); dmin = np.inf
    for k in range(n - 1, -1, -1):
        dmin = min(dmin, a[k, k])
        rinv[k] = 1.0 / max(a[k, k], clamp)
        l = a[k, :k] * rinv[k]
        a[:k, :k] -= np.outer(l, a[k, :k])
        Lm[k, :k] = l
    for k in range(n - 1, 0, -1):
        x[:k] -= Lm[k, :k] * x[k]
    x *= rinv
    for j in range(n - 1):
        x[j + 1:] -= Lm[j + 1:, j] * x[j]
    return x, dmin


def semidefinite_system(rng, par):
    """positive semi-definite A with dof n-1 an exact copy of dof n-2 (equal rows and columns, entries doubles): the first pivot
    of the bottom-up elimination is regular, the second one is exactly zero and meets the clamp"""
    n = len(par)
    B = make_system(rng, par[:n - 1], 1e2, 1)
    B = B / B[n - 2, n - 2]                 # the copied diagonal entry is exactly 1: l = 1 and the next pivot is 1 - 1 * 1 = 0, no rounding
    A = np.zeros((n, n))
    A[:n - 1, :n - 1] = B
    A[n - 1, :n - 1] = B[n - 2]; A[:n - 1, n - 1] = B[n - 2]; A[n - 1, n - 1] = B[n - 2, n - 2]
    return A
