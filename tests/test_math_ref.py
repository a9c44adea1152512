"""The references, input sets and restatements of tests/math_ref.py are sound before any device is involved (CPU tier).

The restated sequences run csrc/dmath.h's arithmetic with a true fma and a modelled hardware seed (the correctly rounded value
times 1 + delta): the bars tests/test_gpu_math.py asserts on the device hold here for every |delta| <= 2^-20, so they do not
rest on the unknown accuracy of v_rcp_f64 / v_rsq_f64."""
import numpy as np
import pytest

import math_ref as R

MP = R.MP


def test_reference_identities_hold_at_200_bits():
    tol = MP.mpf(2) ** -190
    for x in [1e-300, 0.3, 1.0, 2.0, 7.25, 1e300]:
        v = MP.mpf(x)
        assert abs((1 / MP.sqrt(v)) ** 2 * v - 1) < tol and abs(MP.sqrt(v) ** 2 / v - 1) < tol and abs((1 / v) * v - 1) < tol
    for x in [1e-9, 0.5, 20.0, 63.99, -41 * float(R.PIO2)]:
        v = MP.mpf(x)
        assert abs(MP.sin(v) ** 2 + MP.cos(v) ** 2 - 1) < tol
    # log(exp(v)) = v through the quaternion references: subquat(exp(v), identity) returns v
    rng = np.random.default_rng(1)
    rows = []
    for ang in [1e-9, 1e-3, 1.0, 3.0]:
        ax = R._unit(rng, 1, 3)[0]
        ax = [MP.mpf(float(t)) for t in ax]; nrm = R._mp_norm(ax); ax = [t / nrm for t in ax]
        q = R._mp_exp(ax, MP.mpf(ang))
        qd = R._mp_mulquat([MP.mpf(1), 0, 0, 0], q)
        s = R._mp_norm(qd[1:]); back = [t / s * 2 * MP.atan2(s, qd[0]) for t in qd[1:]]
        assert max(abs(b - a * ang) for a, b in zip(ax, back)) < tol * 4
    # the Exact triple reproduces the value: hi + lo to 2^-100, ulp the spacing at the value
    e = R.ref_rcp(np.array([3.0, 1.0, 0.75]))
    assert abs(MP.mpf(e.hi[0]) + MP.mpf(e.lo[0]) - MP.mpf(1) / 3) < MP.mpf(2) ** -100
    assert e.ulp[0] == 2.0 ** -54 and e.ulp[1] == 2.0 ** -52 and e.ulp[2] == 2.0 ** -52
    assert R.ulp_error(np.array([np.nextafter(1.0, 2.0)]), R.ref_rcp(np.array([1.0])))[0] == 1.0


@pytest.mark.parametrize("fn", ["rcp", "rsqrt", "sqrt", "div"])
def test_input_sets_hold_what_they_claim(fn):
    c = R.scalar_classes(fn)
    assert set(c) == {"random", "powers_of_two", "around_one_and_squares", "call_sites", "rounding_boundary"}
    for name, (x, y) in c.items():
        assert 0 < x.size <= 20000 and np.isfinite(x).all() and (x >= 2.2250738585072014e-308).all(), name
        assert (y is None) == (fn != "div")
    x, y = c["rounding_boundary"]
    assert x.size >= 200                                  # enough candidates survive the exact test
    # checked independently at 200 bits: the result sits within 2^-60 (relative) of the midpoint between two doubles
    ex = {"rcp": R.ref_rcp, "rsqrt": R.ref_rsqrt, "sqrt": R.ref_sqrt}[fn](x[:64]) if fn != "div" else R.ref_div(x[:64], y[:64])
    frac = np.abs(ex.lo) / ex.ulp
    assert (np.abs(frac - 0.5) < 2.0 ** -7).all(), np.abs(frac - 0.5).max()      # 2^-60 relative is < 2^-7 of an ulp
    assert np.random.default_rng(0).random() == np.random.default_rng(0).random() and R.scalar_classes(fn) is c     # deterministic, cached


DELTAS = [0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -30, -2.0 ** -27]


@pytest.mark.parametrize("fn", ["rcp", "rsqrt", "sqrt", "div"])
def test_restated_sequences_meet_the_device_bars_for_any_seed_within_2_pow_minus_20(fn):
    worst = {}
    for name, (x, y) in R.scalar_classes(fn).items():
        x = x[:1500]; y = None if y is None else y[:1500]
        exact = {"rcp": R.ref_rcp, "rsqrt": R.ref_rsqrt, "sqrt": R.ref_sqrt}[fn](x) if fn != "div" else R.ref_div(x, y)
        seed_exact = R.ref_rcp(y) if fn == "div" else (R.ref_rcp(x) if fn == "rcp" else (exact if fn == "rsqrt" else R.ref_rsqrt(x)))
        for d in DELTAS:
            seed = R.seed_of(seed_exact, d)
            forms = {"rcp": [lambda: R.seq_rcp(x, seed)], "div": [lambda: R.seq_div(x, y, seed)],
                     "rsqrt": [lambda: R.seq_rsqrt(x, seed, fused=0), lambda: R.seq_rsqrt(x, seed, fused=1)],
                     "sqrt": [lambda: R.seq_sqrt(x, seed, fused=0), lambda: R.seq_sqrt(x, seed, fused=1)]}[fn]
            for f in forms:
                worst[name] = max(worst.get(name, 0.0), np.abs(R.ulp_error(f(), exact)).max())
    print(fn, {k: round(float(v), 3) for k, v in worst.items()})
    bar = 3.0 if fn == "rsqrt" else 1.0
    assert max(worst.values()) <= bar, worst
    # one Newton step fewer misses the bar with the 2^-20 seed: the test can see a dropped step
    if fn == "rcp":
        x = R.scalar_classes(fn)["random"][0][:500]
        ex = R.ref_rcp(x)
        assert np.abs(R.ulp_error(R.seq_rcp(x, R.seed_of(ex, 2.0 ** -20), steps=1), ex)).max() > 100


def test_sincos_restatements_give_the_maxima_the_device_bar_is_set_from():
    got = {}
    for form, fused in (("uncontracted", 0), ("fused", 1)):
        worst, arg = 0.0, None
        for name, x in R.sincos_classes().items():
            es, ec = R.ref_sincos(x)
            s, c = R.seq_sincos(x, fused)
            for g, e in ((s, es), (c, ec)):
                ex = R.sincos_excess(g, e)
                if ex.max() > worst:
                    worst, arg = float(ex.max()), (name, float(x[ex.argmax()]))
        got[form] = worst
        print(form, worst, arg)
    for form in got:
        # the recorded maxima are what this measures (rounded up to 0.01)
        assert got[form] <= R.SINCOS_CPU_MAX[form] and got[form] > R.SINCOS_CPU_MAX[form] - 0.02, got
    # relative error is unbounded next to the multiples of pi/2 and the absolute term covers it: the worst raw error there
    x = R.sincos_classes()["k_pio2"]
    es, ec = R.ref_sincos(x)
    s, c = R.seq_sincos(x, 0)
    small = np.minimum(np.abs(es.hi), np.abs(ec.hi)) < 1e-10
    err = np.where(np.abs(es.hi) < np.abs(ec.hi), np.abs((s - es.hi) - es.lo), np.abs((c - ec.hi) - ec.lo))
    print("absolute error next to k pi/2:", err[small].max())
    assert small.sum() >= 2 * R.KMAX and err[small].max() <= R.SINCOS_ABS
    # a flipped quadrant bit is seen
    s1, c1 = R.seq_sincos(x, 0, qflip=1)
    assert np.abs(s1 - es.hi).max() > 0.5


@pytest.mark.parametrize("n", [18, 27, 33])
def test_ldl_restatement_meets_the_backward_bar_and_no_pivot_is_near_the_clamp(n):
    A, b, cls, trees, conds = R.ldl_systems(n)
    names = list(R.CONDS)
    worst = {}
    for s in range(A.shape[0]):
        x, dmin = R.ldl_numpy(A[s], b[s])
        assert dmin > 1e-12                               # the D_MINVAL clamp is not in play where accuracy is judged
        eta = R.backward_error(A[s], x, b[s])
        assert eta <= R.eta_bar(n)
        lo, hi = conds[s]
        target = R.CONDS[names[cls[s]]]
        assert target / 10 <= lo and hi <= target * 10, (names[cls[s]], lo, hi)          # "about" the class: within a decade
        worst[names[cls[s]]] = max(worst.get(names[cls[s]], 0.0), eta / R.eta_bar(n))
        hi_x, lo_x = R.exact_solution(A[s], b[s])
        assert np.abs(x - hi_x).max() <= conds[s, 1] * R.eta_bar(n) * np.abs(hi_x).max()
        if trees[s]:                                      # the level order is given matrices of M's pattern only
            par = R.dof_parent(n)
            for i in range(n):
                anc, a = set(), i
                while a >= 0:
                    anc.add(a); a = par[a]
                assert all(A[s, i, j] == 0 for j in range(i) if j not in anc)
    print(n, "eta / bar per class:", worst)


def test_exact_residual_and_condition_bounds():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((6, 6)); A = A @ A.T + np.eye(6); x = rng.standard_normal(6)
    b = A @ x
    r = R.exact_residual(A, x, b)
    want = [float(sum(-MP.mpf(A[i, j]) * MP.mpf(x[j]) for j in range(6)) + MP.mpf(b[i])) for i in range(6)]
    assert (r == np.array(want)).all()
    lo, hi = R.cond_inf(A)
    c = np.abs(A).sum(1).max() * np.abs(np.linalg.inv(A)).sum(1).max()
    assert lo <= c * (1 + 1e-9) and c * (1 - 1e-9) <= hi and hi / lo < 1 + 1e-5


def test_clamp_class_meets_exactly_one_zero_pivot():
    for n in (18, 27, 33):
        A = R.semidefinite_system(np.random.default_rng(n), R.dof_parent(n))
        x, dmin = R.ldl_numpy(A, np.ones(n))
        assert dmin == 0.0 and np.isfinite(x).all()
        assert np.linalg.matrix_rank(A) == n - 1
