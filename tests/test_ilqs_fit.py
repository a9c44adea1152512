"""CPU tier of the iLQS planner (no GPU): the spline fit of the conversion (mjpc_hip::SplineFit through cplanner.ilqs_spline_fit) against
the sequential mirror bit for bit and against numpy.linalg.lstsq, splines that come back, the singular cases, the mirror's operator cache,
and the table of ActionFromPolicy's sources."""
import itertools

import numpy as np
import pytest

import gradient_planner_mirror as gm
import ilqs_planner_mirror as sm
from mujoco_mpc_amd import cplanner

SHAPES = [(7, 3), (15, 4), (35, 6)]           # (H - 1, P)
REPRESENTATIONS = [1, 2]                      # linear, cubic
NUS = [1, 3]
DT, T0 = 0.01, 0.3

# Largest relative difference (max |a - b| / max |b|) of the sequential mirror against numpy.linalg.lstsq on the same kron-free system over
# SHAPES x REPRESENTATIONS x NUS with the actions of _case(): measured on the CPU, 1.007e-15 (printed by the lstsq test).  lstsq solves by SVD, the
# fit by the normal equations in another summation order: 100 x that is allowed.
MEASURED_MIRROR_VS_LSTSQ = 1.007e-15
TOLERANCE = 100 * MEASURED_MIRROR_VS_LSTSQ


def _times(H1, P, t0=T0, dt=DT):
    conv = sm.SplineConversion(np.array([[-1.0, 1.0]]), dt)
    kt = conv.knot_times(t0, H1 + 1, P)
    at = [t0]
    for _ in range(H1 - 1):
        at.append(at[-1] + dt)
    return np.array(kt), np.array(at)


def _case(rep, H1, P, nu):
    kt, at = _times(H1, P)
    u = np.random.default_rng(1000 * rep + 10 * H1 + nu).uniform(-1.0, 1.0, (H1, nu))
    return kt, at, u


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


CASES = list(itertools.product(REPRESENTATIONS, SHAPES, NUS))


@pytest.mark.parametrize("rep,shape,nu", CASES)
def test_fit_is_bit_equal_to_the_sequential_mirror(rep, shape, nu):
    kt, at, u = _case(rep, *shape, nu)
    got = cplanner.ilqs_spline_fit(rep, kt, at, u)
    want = sm.spline_fit(rep, kt, at, u)
    assert got is not None and want is not None
    assert np.array_equal(got, want)


def test_fit_agrees_with_lstsq():
    worst_mirror = worst_cpp = 0.0
    for rep, shape, nu in CASES:
        kt, at, u = _case(rep, *shape, nu)
        M = gm.spline_mapping(rep, 1, kt, at)
        ref = np.linalg.lstsq(M, u, rcond=None)[0]
        worst_mirror = max(worst_mirror, _rel(sm.spline_fit(rep, kt, at, u), ref))
        worst_cpp = max(worst_cpp, _rel(cplanner.ilqs_spline_fit(rep, kt, at, u), ref))
    print("largest relative difference against lstsq: mirror %.3e, C++ %.3e; allowed %.3e" % (worst_mirror, worst_cpp, TOLERANCE))
    assert worst_cpp <= TOLERANCE and worst_mirror <= TOLERANCE


@pytest.mark.parametrize("rep,shape,nu", CASES)
def test_actions_on_a_spline_come_back(rep, shape, nu):
    """a constant, and the samples M theta of a spline with knots theta (for the linear representation: of a linear spline with those knots)"""
    H1, P = shape
    kt, at = _times(H1, P)
    const = np.tile(np.linspace(0.25, 0.75, nu), (H1, 1))
    got = cplanner.ilqs_spline_fit(rep, kt, at, const)
    print("constant: relative difference %.3e" % _rel(got, np.tile(const[0], (P, 1))))
    assert _rel(got, np.tile(const[0], (P, 1))) <= TOLERANCE
    theta = np.random.default_rng(7 + P + nu).uniform(-1.0, 1.0, (P, nu))
    u = gm.spline_mapping(rep, 1, kt, at) @ theta
    if rep == 1:            # the samples of the linear spline itself, through the interpolation of GradientPolicy::Action
        u = np.array([gm.interpolate(1, float(t), kt, theta) for t in at])
    got = cplanner.ilqs_spline_fit(rep, kt, at, u)
    print("spline samples: relative difference %.3e" % _rel(got, theta))
    assert _rel(got, theta) <= TOLERANCE


def test_singular_cases_are_refused():
    # linear with P = H: a knot at every step, the last one a step behind the last action (times exact in binary: the column is exactly zero)
    H = 8
    kt = 0.5 + 0.125 * np.arange(H); at = 0.5 + 0.125 * np.arange(H - 1)
    u = np.ones((H - 1, 2))
    assert cplanner.ilqs_spline_fit(1, kt, at, u) is None and sm.spline_fit(1, kt, at, u) is None
    # zero-order: the last knot's column is zero for every shape
    for H1, P in SHAPES:
        kt, at = _times(H1, P)
        u = np.ones((H1, 1))
        assert cplanner.ilqs_spline_fit(0, kt, at, u) is None and sm.spline_fit(0, kt, at, u) is None
    # out of range
    kt, at = _times(7, 3)
    assert cplanner.ilqs_spline_fit(3, kt, at, np.ones((7, 1))) is None
    assert cplanner.ilqs_spline_fit(1, np.arange(26.0), np.arange(40.0) * 0.5, np.ones((40, 1))) is None


def test_the_mirrors_conversion_reuses_the_first_operator_until_the_dimensions_change():
    H, P, nu = 16, 4, 2
    conv = sm.SplineConversion(np.array([[-1.0, 1.0]] * nu), DT)
    rng = np.random.default_rng(3)
    at = T0 + DT * np.arange(H); u = rng.uniform(-0.5, 0.5, (H, nu))
    kt1, k1 = conv.convert(1, T0, H, P, at, u)
    assert conv.cache_miss
    W1 = conv.W
    assert np.array_equal(k1, np.clip(sm.spline_fit(1, kt1, at[:H - 1], u[:H - 1]), -1.0, 1.0))
    # shifted times, same dimensions: the first W, although a fresh one would belong to other times
    shift = 0.0137
    u2 = rng.uniform(-0.5, 0.5, (H, nu))
    kt2, k2 = conv.convert(1, T0 + shift, H, P, at + shift, u2)
    assert not conv.cache_miss and conv.W is W1
    assert kt2[0] == T0 + shift
    assert np.array_equal(k2, np.clip(sm.fit_apply(W1, u2[:H - 1]), -1.0, 1.0))
    # another horizon, another representation: recomputed
    conv.convert(1, T0, H - 4, P, at, u)
    assert conv.cache_miss and conv.W.shape == (P, H - 5)
    conv.convert(2, T0, H - 4, P, at, u)
    assert conv.cache_miss
    # a singular fit caches nothing
    with pytest.raises(sm.SingularFit):
        conv.convert(0, T0, H, P, at, u)
    assert conv.key is None
    # the knots are clamped to the ctrlrange
    _, k3 = conv.convert(1, T0, H, P, at, 5.0 * np.ones((H, nu)))
    assert np.all(k3 == 1.0)


def test_action_from_policy_source_table():
    S, L = sm.kSampling, sm.kiLQG
    table = {
        (S, S, False): sm.SAMPLING_CURRENT, (S, L, False): sm.ILQG_CURRENT, (L, S, False): sm.SAMPLING_CURRENT, (L, L, False): sm.ILQG_CURRENT,
        (S, S, True): sm.SAMPLING_PREVIOUS,       # sampling's policy is updated by every call
        (S, L, True): sm.SAMPLING_PREVIOUS,
        (L, S, True): sm.ILQG_CURRENT,            # the early return left iLQG as it was: its current policy is the previous one
        (L, L, True): sm.ILQG_PREVIOUS,
    }
    assert (sm.SAMPLING_CURRENT, sm.SAMPLING_PREVIOUS, sm.ILQG_CURRENT, sm.ILQG_PREVIOUS) == (0, 1, 2, 3)
    for (prev, act, use_previous), want in table.items():
        assert cplanner.ilqs_action_source(prev, act, use_previous) == want, (prev, act, use_previous)
        assert sm.action_source(prev, act, use_previous) == want, (prev, act, use_previous)


def test_the_planner_class_and_its_c_symbols_exist():
    L = cplanner.lib()
    for name in ("create", "destroy", "reset", "set_state", "set_task", "optimize_policy", "nominal_trajectory", "action_from_policy", "best_trajectory",
                 "values", "timings", "sampling", "ilqg", "spline_fit"):
        assert hasattr(L, "mjpc_ilqs_" + name), name
    assert cplanner.iLQSPlanner._prefix == "mjpc_ilqs_"
