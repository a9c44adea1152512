"""The device's scalar maths (csrc/dmath.h) and linear solves (csrc/linalg.h, csrc/noslip.h) against exact references of their
own (tests/math_ref.py): tests/hip/math_hooks.hip runs each function in isolation, element-wise or one wave per system; this
test builds it into a library of its own and compares bit patterns with 200-bit values and exact residuals.

Every asserted bar stands next to the device maximum measured on an MI355X and the argument that gave it (SCALAR, QUAT, EDGE,
LDL_MEASURED, ...); each test prints the figures it measures before it asserts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import math_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "math_hooks.hip")
SO = os.path.join(ROOT, "tests", "hip", "libmjpc_hip_mathhooks.so")
CSRC = os.path.join(ROOT, "mujoco_mpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FN = {"fast_rsqrt": 0, "fast_rcp": 1, "d_div": 2, "d_sqrt": 3, "d_pow_small": 4, "d_sincos": 5, "seed_rsq": 6, "seed_rcp": 7, "pow": 8}
VF = {"normalize4": 0, "axisangle2quat": 1, "quatintegrate": 2, "subquat": 3, "quat2mat": 4, "normalize3": 5}
LM_FUSED, LM_ROW, LM_SPLIT = 0, 1, 2
NAN = float("nan")


def build_hooks():
    """the flags of __graft_entry__.build_test_hooks(); rebuilt when the source or a kernel header is newer"""
    srcs = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-shared", "-Wno-unused-result",
                               "-Wno-unused-value", "-o", tmp, SRC], cwd=os.path.dirname(SRC))
        os.replace(tmp, SO)
    return SO


_lib = []


def lib():
    if not _lib:
        l = ctypes.CDLL(build_hooks())
        l.mjpc_hip_mathhooks_last_error.restype = ctypes.c_char_p
        _lib.append(l)
    return _lib[0]


def _p(a): return a.ctypes.data_as(ctypes.c_void_p)
def _f(a): return np.ascontiguousarray(a, dtype=np.float64)
def _i(a): return np.ascontiguousarray(a, dtype=np.int32)
def _ok(rc):
    """a HIP error ends the session: nothing more is started on a device that has reported a fault"""
    if rc == -2:
        pytest.exit("HIP error in a math hook: " + lib().mjpc_hip_mathhooks_last_error().decode(), returncode=3)
    assert rc == 0, lib().mjpc_hip_mathhooks_last_error().decode()


def scalar(fn, x, y=None):
    """device results of one element-wise launch as doubles: (first output, second output)"""
    x = _f(x); y = _f(np.ones_like(x) if y is None else y)
    o0, o1 = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size, dtype=np.uint64)
    _ok(lib().mjpc_hip_math_scalar(FN[fn], x.size, _p(x), _p(y), _p(o0), _p(o1), 0))
    return o0.view(np.float64), o1.view(np.float64)


def vector(fn, rows):
    rows = _f(rows); out = np.zeros((rows.shape[0], 9), dtype=np.uint64)
    _ok(lib().mjpc_hip_math_vector(VF[fn], rows.shape[0], _p(rows), _p(out), 0))
    return out.view(np.float64)


# ---- scalar accuracy: asserted bar | device maximum measured on an MI355X, in ulps of the exact value | the argument ------------
SINCOS_B = max(R.SINCOS_CPU_MAX.values()) + 0.5          # the device's contraction pattern is neither restatement: + 0.5 ulp
SCALAR = {
    # header claim "~1 ulp": asserted as 1.0 ulp
    "fast_rcp":   dict(bar=1.0, measured=0.5000, at=0.9999999999999986),
    "d_div":      dict(bar=1.0, measured=0.5000, at=(0.6660382921459077, "a power of two")),
    "d_sqrt":     dict(bar=1.0, measured=0.5771, at=2.759737614603324e-308),      # above 0.5 only below 2^-969: x - s*s is denormal there
    # "full fp64 accuracy" is not a number: bar = measured device maximum + 0.5 ulp (seed may differ between steppings), <= 3
    "fast_rsqrt": dict(bar=1.7111 + 0.5, measured=1.7111, at=3.340584098894289e+61),
    # |err| <= B ulp + 4.2e-25; B = the CPU restatements' maximum (math_ref.SINCOS_CPU_MAX) + 0.5
    "d_sincos":   dict(bar=SINCOS_B, measured=1.4636, at=("sin", 57.33802827302554)),
    # generic powers go to the device's pow: bar = its measured error + 0.5 ulp
    "pow":        dict(bar=1.2162 + 0.5, measured=1.2162, at=(0.16139788056678384, 4.0)),
    # raw hardware seeds, maximum relative error over 4000 random normal arguments: recorded, never asserted
    "seed_rsq":   dict(bar=None, measured=4.648e-08, at=4.962331641127097e+213),  # 2^-24.36
    "seed_rcp":   dict(bar=None, measured=4.342e-08, at=6.857584442713244e+302),  # 2^-24.46
}
REFS = {"fast_rcp": ("rcp", R.ref_rcp), "fast_rsqrt": ("rsqrt", R.ref_rsqrt), "d_sqrt": ("sqrt", R.ref_sqrt), "d_div": ("div", R.ref_div)}


@pytest.mark.parametrize("fn", ["fast_rcp", "d_div", "d_sqrt", "fast_rsqrt"])
def test_scalar_sequences_stay_within_their_bar_of_the_exact_value(fn):
    key, ref = REFS[fn]
    worst, arg = 0.0, None
    for name, (x, y) in R.scalar_classes(key).items():
        got = scalar(fn, x, y)[0]
        err = np.abs(R.ulp_error(got, ref(x, y) if y is not None else ref(x)))
        assert np.isfinite(err).all(), name
        k = int(err.argmax())
        print(f"{fn} {name}: {x.size} arguments, max {err[k]:.4f} ulp at {x[k]!r}" + (f" / {y[k]!r}" if y is not None else ""))
        if err[k] > worst:
            worst, arg = float(err[k]), (name, float(x[k]))
    print(f"{fn}: device maximum {worst:.4f} ulp at {arg}, asserted bar {SCALAR[fn]['bar']}")
    assert worst <= SCALAR[fn]["bar"]


def test_raw_seeds_are_recorded():
    """relative accuracy of v_rcp_f64 / v_rsq_f64 on the accuracy classes: a figure for SCALAR, no assertion on it"""
    for fn, key, ref in (("seed_rcp", "rcp", R.ref_rcp), ("seed_rsq", "rsqrt", R.ref_rsqrt)):
        x = R.scalar_classes(key)["random"][0][:4000]
        got = scalar(fn, x)[0]
        e = ref(x)
        rel = np.abs((got - e.hi) - e.lo) / np.abs(e.hi)
        print(f"{fn}: max relative error {rel.max():.3e} = 2^{np.log2(rel.max()):.2f} at {x[rel.argmax()]!r}")
        assert np.isfinite(got).all()


def test_sincos_stays_within_b_ulp_plus_the_derived_absolute_term():
    worst, arg = 0.0, None
    for name, x in R.sincos_classes().items():
        s, c = scalar("d_sincos", x)
        es, ec = R.ref_sincos(x)
        for what, g, e in (("sin", s, es), ("cos", c, ec)):
            ex = R.sincos_excess(g, e)
            k = int(ex.argmax())
            print(f"d_sincos {name} {what}: max {ex[k]:.4f} ulp beyond {R.SINCOS_ABS} at {x[k]!r}; max |err| {np.abs((g - e.hi) - e.lo).max():.3e}")
            if ex[k] > worst:
                worst, arg = float(ex[k]), (name, what, float(x[k]))
    print(f"d_sincos: device maximum {worst:.4f} ulp at {arg}, asserted bar {SINCOS_B}")
    assert worst <= SINCOS_B


def test_sincos_quadrants_have_the_right_sign_and_swap_for_every_k():
    """at the multiples of pi/2 a wrong sin / cos swap or sign is an error of 1, between them (|sin| = |cos|) a wrong sign is
    an error of 1.4: both sides of every boundary, every |k| <= 41, negative k included"""
    c = R.sincos_classes()
    x = np.concatenate([c["k_pio2"], c["k_half_pio2"], c["rint_decision"]])
    k = np.rint(x / (np.pi / 2))
    assert set(range(-R.KMAX + 1, R.KMAX)) <= set(int(v) for v in k) and (x < 0).sum() > 100
    s, cs = scalar("d_sincos", x)
    es, ec = R.ref_sincos(x)
    err = np.maximum(np.abs(s - es.hi), np.abs(cs - ec.hi))
    print(f"quadrants: {x.size} arguments, max |err| {err.max():.3e}")
    assert err.max() < 1e-12


def test_sincos_across_64_stays_within_the_bar_of_both_paths():
    x = np.concatenate([R.sincos_classes()["below_64"], R.SINCOS_LIBM_CLASS])
    s, c = scalar("d_sincos", x)
    es, ec = R.ref_sincos(x)
    ex = np.maximum(R.sincos_excess(s, es), R.sincos_excess(c, ec))
    print("d_sincos across 64:", dict(zip(x.tolist(), np.round(ex, 3).tolist())))
    assert ex.max() <= SINCOS_B


def test_pow_small_multiplies_for_1_2_3_and_is_the_device_pow_otherwise():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(0.0, 1.0, 2000), rng.uniform(0, 100.0, 2000), 10.0 ** rng.uniform(-100, 100, 500)])
    for p, want in ((1.0, x), (2.0, x * x), (3.0, (x * x) * x)):
        got = scalar("d_pow_small", x, np.full_like(x, p))[0]
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), p
    worst, arg = 0.0, None
    xs = x[:4000]
    for p in (0.5, 1.5, 2.5, 4.0, -2.0):
        pp = np.full_like(xs, p)
        got, ref = scalar("d_pow_small", xs, pp)[0], scalar("pow", xs, pp)[0]
        assert (got.view(np.uint64) == ref.view(np.uint64)).all(), p
        err = np.abs(R.ulp_error(ref, R.ref_pow(xs, pp)))
        if err.max() > worst:
            worst, arg = float(err.max()), (p, float(xs[err.argmax()]))
    print(f"device pow: maximum {worst:.4f} ulp at {arg}, asserted bar {SCALAR['pow']['bar']}")
    assert worst <= SCALAR["pow"]["bar"]


# ---- edge class: one table of (function, argument) -> device result --------------------------------------------------------------
# Where the device gives the IEEE result nothing is listed; every deviation is listed exactly as the MI355X gives it (DESIGN.md,
# "Domains of the fast scalar sequences", names them and the guards of the call sites).  The domain of all four sequences is the
# normal doubles (fast_rcp / d_div: |x| from 2^-1022 to the largest double; fast_rsqrt / d_sqrt: positive x); an argument inside it
# is held to the accuracy bar, not to a bit pattern.
INF = float("inf")
EDGE_DEVIATIONS = [          # (function, argument, device result)
    # v_rcp_f64 gives inf / 0 / inf for these and the Newton steps turn them into NaN (0 * inf)
    ("fast_rcp", 0.0, NAN), ("fast_rcp", -0.0, NAN), ("fast_rcp", INF, NAN), ("fast_rcp", -INF, NAN),
    ("fast_rcp", 5e-324, NAN), ("fast_rcp", -5e-324, NAN), ("fast_rcp", 1e-310, NAN),
    ("d_div", 0.0, NAN), ("d_div", -0.0, NAN), ("d_div", INF, NAN), ("d_div", -INF, NAN),
    ("d_div", 5e-324, NAN), ("d_div", -5e-324, NAN), ("d_div", 1e-310, NAN),
    # !(x > 0) -> 0 by contract (T = x * rsqrt(x) = 0); inf -> NaN; denormal arguments lose the bits 0.5 * x drops
    ("fast_rsqrt", 0.0, 0.0), ("fast_rsqrt", -0.0, 0.0), ("fast_rsqrt", INF, NAN), ("fast_rsqrt", -INF, 0.0), ("fast_rsqrt", NAN, 0.0),
    ("fast_rsqrt", -5e-324, 0.0), ("fast_rsqrt", -1.7976931348623157e308, 0.0), ("fast_rsqrt", -1.0, 0.0), ("fast_rsqrt", -1e-300, 0.0),
    ("fast_rsqrt", 5e-324, 1.0122556037722192e+162), ("fast_rsqrt", 2.225073858507201e-308, 6.703903964971299e+153),
    ("fast_rsqrt", 1e-310, 9.999999999999768e+154), ("fast_rsqrt", 5.6e-309, 1.3363062095621215e+154),
    # -0 -> +0; inf -> NaN (inf * rsqrt(inf)); the smallest denormals come out wrong, even negative
    ("d_sqrt", -0.0, 0.0), ("d_sqrt", INF, NAN), ("d_sqrt", 5e-324, -5.001207186341424e-162), ("d_sqrt", 1e-310, 9.999999999999984e-156),
]
EDGE_REFS = {"fast_rcp": R.ref_rcp, "d_div": R.ref_rcp, "fast_rsqrt": R.ref_rsqrt, "d_sqrt": R.ref_sqrt}
TINY = 2.2250738585072014e-308


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


def test_edge_arguments_give_the_ieee_result_or_the_recorded_deviation():
    x = R.EDGE_ARGS
    with np.errstate(all="ignore"):
        ieee = {"fast_rcp": 1.0 / x, "fast_rsqrt": 1.0 / np.sqrt(x), "d_sqrt": np.sqrt(x), "d_div": 1.0 / x}
    bad, seen = [], set()
    for fn, want in ieee.items():
        got = scalar(fn, np.ones_like(x), x)[0] if fn == "d_div" else scalar(fn, x)[0]
        for a, g, w in zip(x.tolist(), got.tolist(), want.tolist()):
            dev = [(k, row[2]) for k, row in enumerate(EDGE_DEVIATIONS) if row[0] == fn and _same(row[1], a)]
            inside = np.isfinite(a) and abs(a) >= TINY and np.isfinite(w) and abs(w) >= TINY
            print(f"edge {fn}({a!r}) = {g!r}   IEEE {w!r}" + ("   (recorded deviation)" if dev else "") + ("   (inside the domain)" if inside else ""))
            if inside:                                         # a normal argument with a normal result: the accuracy bar
                assert not dev
                if not abs(R.ulp_error(np.array([g]), EDGE_REFS[fn](np.array([a])))[0]) <= SCALAR[fn]["bar"]: bad.append((fn, a, g, w))
            elif not _same(g, dev[0][1] if dev else w): bad.append((fn, a, g, dev[0][1] if dev else w))
            seen.update(k for k, _ in dev)
    assert seen == set(range(len(EDGE_DEVIATIONS)))                        # no stale row in the table
    s, c = scalar("d_sincos", x)
    for a, gs, gc in zip(x.tolist(), s.tolist(), c.tolist()):
        print(f"edge d_sincos({a!r}) = {gs!r}, {gc!r}")
        if np.isfinite(a):                                     # (IEEE here: the correctly rounded value to the d_sincos bar)
            es, ec = R.ref_sincos(np.array([a]))
            if not (R.sincos_excess(np.array([gs]), es)[0] <= SINCOS_B and R.sincos_excess(np.array([gc]), ec)[0] <= SINCOS_B): bad.append(("d_sincos", a, gs, gc))
        elif not (np.isnan(gs) and np.isnan(gc)): bad.append(("d_sincos", a, gs, gc))
    assert not bad, bad


# ---- quaternion helpers ----------------------------------------------------------------------------------------------------------
# Bars in units of 2^-53 of the result's norm: the number of roundings on the longest path times the per-operation bar (2 units
# per rounding: one correctly rounded operation is half an ulp, an ulp is at most 2 x 2^-53 of the value; the sequences above
# are asserted to 1 .. 2 ulp and count as 2 .. 4 roundings).
#   normalize4: 7 for the sum of squares (halved by the root), 4 for fast_rsqrt, 1 product: 9 roundings
#   axisangle2quat: 1 for angle / 2 (exact) + d_sincos (B ulp = 4 roundings) + 1 product; the argument error of an angle up to
#     10 pi is not the helper's: angles are exact doubles here: 5 roundings
#   quatintegrate: normalize3 (7 / 2 + sqrt + reciprocal + product = 7) + angle (1 + 3.5 carried from the norm, times the
#     angle <= pi: 14) + axisangle2quat (5) + normalize4 (9) + mulquat (4 products + 3 sums = 7, on operands carrying 9 and 26)
#     + the closing normalize4 (9): 24 + 26 + 7 + 9 = 66 roundings
#   subquat: mulquat (7) + normalize3 (7) + atan2 (2) + 2 products, relative to max(|result|, pi): next to the antipode the
#     2 pi wrap cancels and leaves the absolute error of a value near 2 pi: 4 x (7 + 7 + 2 + 2) = 72 at most
#   quat2mat: 4 products + 3 sums on |q|^2: 7 roundings
QUAT = {
    "normalize4":     dict(bar=2 * 9, measured=8.034, at="norm 0.999999999999999: left alone below the D_MINVAL switch"),
    "axisangle2quat": dict(bar=2 * 5, measured=0.614, at="angle 0.001"),
    "quatintegrate":  dict(bar=2 * 66, measured=6.853, at="angle pi, norm 0.999999999999999"),
    "subquat":        dict(bar=2 * 72, measured=1.512, at="angle pi - 1e-3"),
    "quat2mat":       dict(bar=2 * 7, measured=1.442, at="unit"),
}


def _quat_err(fn):
    inp, labels = R.quat_inputs(fn)
    width = {"subquat": 3, "quat2mat": 9}.get(fn, 4)
    got = vector(fn, inp)[:, :width]
    hi, lo = getattr(R, "ref_" + fn)(inp)
    d = np.abs((got - hi) - lo).max(axis=1)
    nrm = np.sqrt((hi * hi).sum(axis=1))
    if fn == "subquat":
        nrm = np.maximum(nrm, np.pi)
    if fn == "quat2mat":
        nrm = (inp[:, :4] ** 2).sum(axis=1)
    err = d / (R.U * nrm)
    k = int(err.argmax())
    print(f"{fn}: {len(labels)} rows, max error {err[k]:.3f} x 2^-53 at '{labels[k]}' {inp[k].tolist()}, asserted bar {QUAT[fn]['bar']}")
    return inp, labels, got, err


@pytest.mark.parametrize("fn", ["normalize4", "axisangle2quat", "quatintegrate", "subquat", "quat2mat"])
def test_quaternion_helpers_against_the_exact_maps(fn):
    inp, labels, got, err = _quat_err(fn)
    assert np.isfinite(got).all()
    assert err.max() <= QUAT[fn]["bar"]
    if fn in ("normalize4", "quatintegrate"):
        # unit to 2 ulp wherever the helper normalised; d_normalize4 leaves |q| within D_MINVAL of 1 alone: bit-identical then
        n = np.array([float(R._mp_norm(R._mpf(q))) for q in got])
        changed = (got != inp[:, :4]).any(axis=1) if fn == "normalize4" else np.ones(len(n), dtype=bool)
        tol = np.where(changed, 2 * 2.0 ** -52, R.D_MINVAL + 2.0 ** -52)
        if fn == "quatintegrate":
            tol = np.full(len(n), R.D_MINVAL + 2.0 ** -52)       # the closing d_normalize4 has the same switch
        print(f"{fn}: | |q| - 1 | max {np.abs(n - 1).max():.3e}, rows left alone {int((~changed).sum())}")
        assert (np.abs(n - 1) <= tol).all()


def test_subquat_of_equal_quaternions_is_exactly_zero():
    """d_subquat(q, q) = 0 exactly.  The vector part of conj(q) q in d_mulquat, q0 q1 - q1 q0 - q2 q3 + q3 q2, is contracted into
    a chain of FMAs on the device and keeps the rounding error of its first product (up to 9.2e-17 measured); d_subquat returns
    zero where that part is below D_MINVAL, where d_normalize3 has no axis to give either."""
    inp, labels, got, _ = _quat_err("subquat")
    eq = got[np.array(labels) == "equal"]
    print(f"subquat of equal quaternions: |r| max {np.abs(eq).max():.3e}, non-zero rows {int((eq != 0).any(axis=1).sum())} of {len(eq)}")
    assert (eq == 0).all()


def test_subquat_of_antipodal_quaternions_wraps_to_zero_and_integrate_at_rest_keeps_q():
    inp, labels, got, _ = _quat_err("subquat")
    lab = np.array(labels)
    anti = np.sqrt((got[lab == "antipodal"] ** 2).sum(axis=1))
    near = np.sqrt((got[np.char.startswith(lab, "nearly")] ** 2).sum(axis=1))
    print(f"subquat antipodal |r| max {anti.max():.3e}, nearly antipodal |r| max {near.max():.3e}")
    assert (anti < 1e-15).all() and (near < 1e-4).all()                                      # wrapped to 0, never 2 pi
    inp, labels, got, _ = _quat_err("quatintegrate")
    lab = np.array(labels)
    rest = (lab == "below D_MINVAL") | (lab == "zero velocity") | (lab == "angle 0.0 norm 1.0")
    assert rest.sum() >= 65
    assert (got[rest].view(np.uint64) == np.ascontiguousarray(inp[rest, :4]).view(np.uint64)).all()   # a unit q is left bit-identical


def test_normalize3_is_the_ieee_norm_and_quotient():
    rng = np.random.default_rng(3)
    v = np.zeros((256, 8)); v[:, :3] = rng.standard_normal((256, 3)) * 10.0 ** rng.uniform(-8, 8, (256, 1))
    v[0, :3] = 0; v[1, :3] = [1e-16, 0, 0]
    got = vector("normalize3", v)[:, :4]
    hi = np.array([[float(t / R._mp_norm(R._mpf(r[:3]))) for t in R._mpf(r[:3])] for r in v[2:]])
    assert np.abs(got[2:, :3] - hi).max() <= 6 * R.U and (got[:2, :3] == [1.0, 0.0, 0.0]).all()
    assert np.abs(got[2:, 3] / np.sqrt((v[2:, :3] ** 2).sum(axis=1)) - 1).max() <= 4 * R.U


# ---- linear solves ---------------------------------------------------------------------------------------------------------------
CLASSES = list(R.CONDS)
# maxima of the backward error eta measured on an MI355X and for numpy.linalg.solve on the same systems, per size and condition
# class (all orders and modes): (device, numpy).  The device must stay within twice this ratio to numpy and under eta_bar(n).
# The register L^T D L loses backward accuracy as the condition number grows (90 x numpy at 1e13, n = 18, level order, system 61 with
# three partials) while IEEE restatements of the same elimination stay at 1 x: measured, under 2 % of eta_bar, not explained.
LDL_MEASURED = {
    (18, '1e2'): (4.979e-17, 4.786e-17), (18, '1e6'): (5.407e-17, 4.370e-17), (18, '1e10'): (1.814e-16, 6.562e-17), (18, '1e13'): (4.574e-15, 5.092e-17),
    (27, '1e2'): (6.068e-17, 3.685e-17), (27, '1e6'): (1.010e-16, 3.810e-17), (27, '1e10'): (1.001e-16, 4.734e-17), (27, '1e13'): (7.894e-16, 3.591e-17),
    (33, '1e2'): (7.791e-17, 4.399e-17), (33, '1e6'): (4.487e-17, 3.347e-17), (33, '1e10'): (1.890e-16, 2.818e-17), (33, '1e13'): (2.328e-16, 4.369e-17),
}
GEN_MEASURED = {
    (1, '1e2'): (4.142e-17, 4.142e-17), (1, '1e6'): (1.376e-16, 2.716e-17), (1, '1e10'): (2.758e-17, 2.758e-17), (1, '1e13'): (1.400e-16, 4.656e-17),
    (2, '1e2'): (1.111e-17, 3.183e-17), (2, '1e6'): (6.022e-17, 2.237e-17), (2, '1e10'): (9.956e-17, 9.512e-17), (2, '1e13'): (1.550e-17, 9.894e-18),
    (3, '1e2'): (1.669e-17, 3.365e-17), (3, '1e6'): (1.565e-17, 1.170e-17), (3, '1e10'): (7.784e-18, 7.539e-18), (3, '1e13'): (2.419e-17, 3.948e-17),
    (15, '1e2'): (1.576e-17, 1.320e-17), (15, '1e6'): (1.064e-17, 1.457e-17), (15, '1e10'): (1.536e-17, 1.880e-17), (15, '1e13'): (9.391e-18, 2.412e-17),
    (16, '1e2'): (1.416e-17, 1.272e-17), (16, '1e6'): (1.161e-17, 2.887e-17), (16, '1e10'): (1.406e-17, 3.768e-17), (16, '1e13'): (3.720e-17, 1.007e-17),
    (17, '1e2'): (9.688e-18, 1.189e-17), (17, '1e6'): (3.031e-17, 1.575e-17), (17, '1e10'): (6.002e-18, 1.173e-17), (17, '1e13'): (1.298e-17, 2.739e-17),
    (31, '1e2'): (1.218e-17, 1.563e-17), (31, '1e6'): (1.157e-17, 2.989e-17), (31, '1e10'): (1.067e-17, 4.053e-17), (31, '1e13'): (1.587e-17, 2.540e-17),
    (32, '1e2'): (3.311e-17, 2.369e-17), (32, '1e6'): (2.043e-17, 2.566e-17), (32, '1e10'): (1.155e-17, 1.259e-17), (32, '1e13'): (1.478e-17, 1.231e-17),
    (33, '1e2'): (2.472e-17, 3.120e-17), (33, '1e6'): (1.403e-17, 3.510e-17), (33, '1e10'): (1.103e-17, 2.182e-17), (33, '1e13'): (1.828e-17, 1.492e-17),
    (63, '1e2'): (5.426e-17, 5.198e-17), (63, '1e6'): (4.406e-18, 1.776e-17), (63, '1e10'): (8.842e-18, 1.869e-17), (63, '1e13'): (1.190e-17, 1.671e-17),
    (64, '1e2'): (6.969e-17, 2.930e-17), (64, '1e6'): (2.821e-17, 1.796e-17), (64, '1e10'): (1.020e-17, 1.517e-17), (64, '1e13'): (6.030e-18, 1.893e-17),
    (65, '1e2'): (3.680e-17, 2.947e-17), (65, '1e6'): (1.236e-17, 2.808e-17), (65, '1e10'): (1.141e-17, 2.130e-17), (65, '1e13'): (1.087e-17, 2.845e-17),
}
SMALL_MEASURED = {
    (5, '1e2'): (4.680e-17, 6.092e-17), (5, '1e6'): (5.856e-17, 3.093e-17),
}


def _runs_of(n):
    """every (system, mode, nx, matrix) the register L^T D L is given: A fused / row / split, and for nx = 1 .. 3 the split
    A0 + X0 (+ X1 + X2) next to the pre-summed ((A0 + X0) + X1) + X2"""
    A, b, cls, trees, conds = R.ldl_systems(n)
    rng = np.random.default_rng(n)
    runs = []           # (system, kind, mode, nx, A given, X given, matrix solved)
    for s in range(A.shape[0]):
        zero = np.zeros((3, n, n))
        for kind, mode in (("fused", LM_FUSED), ("row", LM_ROW), ("split", LM_SPLIT)):
            runs.append((s, kind, mode, 0, A[s], zero, A[s]))
        mask = A[s] != 0
        X = np.stack([(lambda g: (g + g.T) * mask * np.abs(A[s]))(rng.standard_normal((n, n))) for _ in range(3)])
        for nx in (1, 2, 3):
            A0 = A[s] - X[:nx].sum(axis=0)
            P = A0.copy()
            for w in range(nx):
                P = P + X[w]
            Xg = np.where(np.arange(3)[:, None, None] < nx, X, NAN)
            runs.append((s, f"extra{nx}", LM_FUSED, nx, A0, Xg, P))
            runs.append((s, f"presum{nx}", LM_FUSED, 0, P, zero, P))
    return runs


_ldl = {}


def ldl_run(n):
    """two launches per size over all runs: pad and spare column 0.0, then NaN; upper triangles always NaN (never read)"""
    if n not in _ldl:
        A, b, cls, trees, conds = R.ldl_systems(n)
        runs = _runs_of(n)
        up = np.triu(np.ones((n, n), dtype=bool), 1)
        Ag = _f(np.stack([np.where(up, NAN, r[4]) for r in runs]))
        Xg = _f(np.stack([np.where(up[None], NAN, r[5]) for r in runs]))
        bg = _f(np.stack([b[r[0]] for r in runs]))
        mode, nx, tree = _i([r[2] for r in runs]), _i([r[3] for r in runs]), _i([trees[r[0]] for r in runs])
        outs = []
        for fill in (0.0, NAN):
            out = np.zeros((len(runs), 2, n), dtype=np.uint64)
            _ok(lib().mjpc_hip_math_ldl(n, len(runs), _p(Ag), _p(Xg), _p(bg), _p(mode), _p(nx), _p(tree), ctypes.c_double(fill), _p(out), 0))
            outs.append(out)
        _ldl[n] = (runs, outs[0], outs[1])
    return _ldl[n]


def _judge(name, n, recs, measured):
    """recs: (class index, certified cond, A, x, b).  Backward error (exact residual) under the derived bar and within twice the
    recorded ratio to numpy's; forward error under cond x the asserted eta; 1e-12 kept for the 1e2 class."""
    dev, ref, fwd, who = {}, {}, {}, {}
    for ci, cond, A, x, b, label in recs:
        assert np.isfinite(x).all()
        eta = R.backward_error(A, x, b)
        if eta > dev.get(ci, 0.0):
            dev[ci], who[ci] = eta, label
        ref[ci] = max(ref.get(ci, 0.0), R.backward_error(A, np.linalg.solve(A, b), b))
        hi, lo = R.exact_solution(A, b)
        f = np.abs((x - hi) - lo).max() / np.abs(hi).max()
        fwd[ci] = max(fwd.get(ci, 0.0), f)
        assert f <= cond * R.eta_bar(n), (name, CLASSES[ci], f, cond)
        if ci == 0:
            assert np.allclose(x, hi, rtol=1e-12, atol=1e-13)
    for ci in sorted(dev):
        print(f"{name} n {n} class {CLASSES[ci]}: eta device {dev[ci]:.3e} numpy {ref[ci]:.3e} ratio {dev[ci] / ref[ci]:.2f} "
              f"bar {R.eta_bar(n):.3e}; forward error {fwd[ci]:.3e}; worst eta at {who[ci]}")
        assert dev[ci] <= R.eta_bar(n)
        if measured.get((n, CLASSES[ci])):
            d0, r0 = measured[(n, CLASSES[ci])]
            assert dev[ci] <= 2 * (d0 / r0) * ref[ci], (name, n, CLASSES[ci], dev[ci], ref[ci])
    print(f"{name} n {n} literal: " + ", ".join(f"({n}, '{CLASSES[ci]}'): ({dev[ci]:.3e}, {ref[ci]:.3e})" for ci in sorted(dev)))


@pytest.mark.parametrize("n", [18, 27, 33])
def test_register_ldl_backward_and_forward_error_in_every_mode_and_order(n):
    A, b, cls, trees, conds = R.ldl_systems(n)
    runs, out, _ = ldl_run(n)
    x = out[:, 0].view(np.float64)
    # every mode and both orders meet the bars independently (dense and level order, fused and split are different eliminations)
    _judge("register LDL", n, [(cls[r[0]], conds[r[0], 1], r[6], x[k], b[r[0]], f"system {r[0]} {r[1]} tree {trees[r[0]]}") for k, r in enumerate(runs)], LDL_MEASURED)
    assert set(trees) == {0, 1}


@pytest.mark.parametrize("n", [18, 27, 33])
def test_register_ldl_bit_equalities_and_poison(n):
    runs, out, out_nan = ldl_run(n)
    at = {(r[0], r[1]): k for k, r in enumerate(runs)}
    nsys = 1 + max(r[0] for r in runs)
    x, negx = out[:, 0], out[:, 1]
    for s in range(nsys):
        # LDLExtra.row: the same elimination from registers
        assert (x[at[s, "row"]] == x[at[s, "fused"]]).all()
        # partials added while loading = the pre-summed matrix
        for nx in (1, 2, 3):
            assert (x[at[s, f"extra{nx}"]] == x[at[s, f"presum{nx}"]]).all(), (s, nx)
    # negx = -x bit for bit where the routine offers it; untouched where it does not
    fused = np.array([r[2] != LM_SPLIT for r in runs])
    assert (negx[fused] == (x[fused] ^ np.uint64(1 << 63))).all()
    assert (negx[~fused] == 0).all()                      # (the hook's own +0.0 fill: the split form has no negx)
    # NaN in the pad behind every block, in the spare columns and above the diagonals reaches no result
    assert (out_nan[:, 0] == out[:, 0]).all() and (out_nan[fused, 1] == out[fused, 1]).all()
    assert not np.isnan(x.view(np.float64)).any()


@pytest.mark.parametrize("n", [18, 27, 33])
def test_register_ldl_clamp_class_follows_the_restated_elimination(n):
    """positive semi-definite A, dof n-1 an exact copy of dof n-2: the second pivot is exactly 0 and becomes D_MINVAL.  Pins what
    the clamp does (it does not judge it): the regular components equal the numpy restatement with the same clamps"""
    rng = np.random.default_rng(100 + n)
    S = 8
    A = np.stack([R.semidefinite_system(rng, R.dof_parent(n)) for _ in range(S)])
    b = rng.standard_normal((S, n)); b[:, n - 1] = b[:, n - 2]           # consistent: the clamped component stays moderate
    b[S // 2:, n - 1] += 1.0                                              # inconsistent: it is 1e15 and must not reach the others
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    for tree in (0, 1):
        out = np.zeros((S, 2, n), dtype=np.uint64)
        _ok(lib().mjpc_hip_math_ldl(n, S, _p(_f(np.where(up, NAN, A))), _p(_f(np.zeros((S, 3, n, n)))), _p(_f(b)), _p(_i([0] * S)), _p(_i([0] * S)),
                                    _p(_i([tree] * S)), ctypes.c_double(NAN), _p(out), 0))
        x = out[:, 0].view(np.float64)
        for s in range(S):
            want, dmin = R.ldl_numpy(A[s], b[s])
            assert dmin == 0.0
            cond = R.cond_inf(A[s][:n - 1, :n - 1])[1]
            d = np.abs(x[s, :n - 2] - want[:n - 2]).max() / np.abs(want[:n - 2]).max()
            print(f"clamp class n {n} tree {tree} set {s}: regular components differ by {d:.3e} (bar {cond * R.eta_bar(n):.3e}), x[n-2] = {x[s, n - 2]:.3e} restated {want[n - 2]:.3e}")
            assert d <= cond * R.eta_bar(n)
            assert np.isfinite(x[s]).all() and abs(x[s, n - 2] - want[n - 2]) <= 1e-6 * abs(want[n - 2]) + 1e-6


GENERIC_N = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65]


@pytest.mark.parametrize("n", GENERIC_N)
def test_generic_lds_cholesky_across_the_lane_stride(n):
    A, b, cls, trees, conds = R.ldl_systems(n, True)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    Ag = _f(np.where(up, NAN, A))
    xs = []
    for fused in (0, 1):
        out = np.zeros((A.shape[0], n), dtype=np.uint64)
        _ok(lib().mjpc_hip_math_chol_lds(n, A.shape[0], fused, _p(Ag), _p(_f(b)), ctypes.c_double(NAN), _p(out), 0))
        xs.append(out)
    assert (xs[0] == xs[1]).all()                                       # chol_factor_solve<0> is the two LDS routines in a row
    x = xs[0].view(np.float64)
    _judge("LDS Cholesky", n, [(cls[s], conds[s, 1], A[s], x[s], b[s], f"system {s}") for s in range(A.shape[0])], GEN_MEASURED)


def test_small_cholesky_of_the_noslip_solver_and_its_rank():
    n, S = 5, 64
    rng = np.random.default_rng(55)
    A, b, conds, cls = [], [], [], []
    for ci, cond in enumerate(list(R.CONDS.values())[:2]):               # mindiag = 1e-10 is a rank decision of its own from 1e10 on
        for _ in range(S // 2 - 8):
            a = R.make_system(rng, R.chain_parent(n), cond, 0)
            a /= np.abs(a).max()
            A.append(a); b.append(rng.standard_normal(n)); conds.append(R.cond_inf(a)[1]); cls.append(ci)
    nfull = len(A)
    for _ in range(S // 4):                                              # rank 4: the last direction copies the one before
        a = R.semidefinite_system(rng, R.chain_parent(n))
        A.append(a); b.append(rng.standard_normal(n))
    A, b = _f(A), _f(b)
    out, rank = np.zeros((len(A), n), dtype=np.uint64), np.zeros(len(A), dtype=np.int32)
    _ok(lib().mjpc_hip_math_small_chol(n, len(A), _p(A), _p(b), ctypes.c_double(1e-10), _p(out), _p(rank), 0))
    x = out.view(np.float64)
    print("small Cholesky ranks:", rank.tolist())
    assert (rank[:nfull] == n).all() and (rank[nfull:] == n - 1).all()
    _judge("small Cholesky", n, [(cls[s], conds[s], A[s], x[s], b[s], f"system {s}") for s in range(nfull)], SMALL_MEASURED)
    assert np.isfinite(x).all()


def test_loader_refuses_a_contact_pair_without_positive_friction():
    """constraint.h and solver.h divide by a contact's friction coefficients with d_div / fast_rcp (NaN at 0) and nothing
    clamps them (MuJoCo's mjMINMU): the loader refuses a pair whose combined coefficient of a used dimension is not positive;
    a coefficient no contact dimension of the model reads (torsional with condim 3) may be zero"""
    from mujoco_mpc_amd.modelgen import quadruped
    from mujoco_mpc_amd.planner import HipBackend
    m, task, _ = quadruped()
    free = int(np.flatnonzero((np.asarray(m["geom_contype"]) == 0) & (np.asarray(m["geom_conaffinity"]) == 0))[0])
    assert int(np.max(m["geom_condim"])) == 6
    fr = np.array(m["geom_friction"], float).reshape(-1, 3)
    for k in range(3):                                   # the feet have condim 6: sliding, torsional and rolling are all read
        bad = dict(m); f = fr.copy(); f[:, k] = 0.0; bad["geom_friction"] = f
        with pytest.raises(RuntimeError) as e:
            HipBackend(bad, task, max_samples=4, max_horizon=4)
        assert "positive friction" in str(e.value) and f"coefficient {k}" in str(e.value), str(e.value)
    # a geom that collides with nothing may have any coefficients
    fine = dict(m); f = fr.copy(); f[free] = 0.0; fine["geom_friction"] = f
    HipBackend(fine, task, max_samples=4, max_horizon=4)
