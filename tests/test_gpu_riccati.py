"""GPU tier of the iLQG backward pass (mjpc_hip_ilqg_backward_pass, mjpc_hip_trajectory_ilqg): the kernel against the host C++ bit for bit at
the shapes of the CPU tier, on the reference's LQR fixture, on the global-scratch path and through the regularisation loop; the fused call
against the composed path; misuse."""
import ctypes as C

import numpy as np
import pytest

import riccati_cases as rc
import transition_cases as tc
from mujoco_mpc_amd import capi, derivatives as D
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

NAMES = ("A", "B", "cx", "cu", "cxx", "cxu", "cuu", "actions", "action_limits")
_engines = {}


@pytest.fixture(scope="module")
def engine():
    """one engine per model for the whole module; the backward pass borrows its device and stream only"""
    def get(name):
        if name not in _engines:
            m, task, _ = tc.model(name)
            _engines[name] = HipBackend(m, task, max_samples=256, max_horizon=2)
        return _engines[name]
    yield get
    for be in _engines.values():
        be.close()
    _engines.clear()


def _both(be, c, reg=None, **kw):
    """(host, device): ILQGBackwardPass.riccati_host from zeros, .compute into NaN-poisoned rows"""
    T, nd = c["cx"].shape; nu = c["cu"].shape[1]
    out = []
    for device in (False, True):
        bp = D.ILQGBackwardPass(nd, nu, T)
        if reg is not None:
            bp.regularization = reg
        args = [c[k] for k in NAMES]
        out.append(bp.compute(be, *args, fill=np.nan, **kw) if device else bp.riccati_host(*args, **kw))
    return out


def _assert_equal(h, g):
    assert list(h["status"]) == list(g["status"])
    assert (h["regularization"], h["regularization_rate"]) == (g["regularization"], g["regularization_rate"])
    for k in rc.OUT_KEYS:
        assert not np.isnan(g[k]).any(), k
        assert np.array_equal(h[k], g[k]), k


@pytest.mark.parametrize("shape", rc.SHAPES, ids=str)
def test_device_equals_host_bit_for_bit(engine, shape):
    be = engine("particle")
    nd, nu, T = rc.shape(shape)
    c = rc.trajectory(nd, nu, T)
    for reg_type in rc.REG_TYPES:
        for limits in (0, 1):
            h, g = _both(be, c, regularization_type=reg_type, action_limits_on=limits)
            assert list(g["status"]) == [1, -1, 0]
            _assert_equal(h, g)
    # the HipBackend call is the same kernel: NULL-free outputs, the settings struct
    o = be.ilqg_backward_pass(*[c[k] for k in NAMES], regularization_type=2, action_limits_on=1)
    h, _ = _both(be, c, regularization_type=2, action_limits_on=1)
    for k in rc.OUT_KEYS:
        assert np.array_equal(o[k], h[k]), k


def test_lqr_fixture(engine):
    be = engine("particle")
    c, exp, tol, reg = rc.lqr()
    h, g = _both(be, c, reg=(reg, 1.0, 2.0))
    _assert_equal(h, g)
    for k, v in exp.items():
        assert np.abs(g[k][:len(v)] - v).max() <= tol, k


def test_global_scratch_path(engine):
    """the smallest nd (at nu = 2) whose work image exceeds the workgroup's LDS: the image lies in the call's global scratch"""
    be = engine("particle")
    lib = capi.load_engine()
    in_lds = C.c_int(1)
    nd = 1
    while lib.mjpc_hip_riccati_layout_bytes(nd, 2, C.byref(in_lds)) > 0 and in_lds.value:
        nd += 1
    assert lib.mjpc_hip_riccati_layout_bytes(nd - 1, 2, C.byref(in_lds)) <= 160 * 1024 and in_lds.value == 1
    assert lib.mjpc_hip_riccati_layout_bytes(nd, 2, C.byref(in_lds)) > 160 * 1024 and in_lds.value == 0
    c = rc.trajectory(nd, 2, 3)
    for limits in (0, 1):
        h, g = _both(be, c, regularization_type=0, action_limits_on=limits)
        assert list(g["status"]) == [1, -1, 0]
        _assert_equal(h, g)


@pytest.mark.parametrize("limits", [0, 1])
def test_regularisation_loop(engine, limits):
    be = engine("particle")
    c, knot = rc.failing_knot()
    h, g = _both(be, c, regularization_type=0, action_limits_on=limits)
    assert list(g["status"]) == [1, -1, 3] and (g["regularization"], g["regularization_rate"]) == (64.0, 8.0)
    _assert_equal(h, g)
    h, g = _both(be, c, regularization_type=0, action_limits_on=limits, max_regularization_iterations=2)
    assert list(g["status"]) == [0, knot, 2] and (g["regularization"], g["regularization_rate"]) == (8.0, 4.0)
    _assert_equal(h, g)


@pytest.mark.parametrize("name,T", [("cartpole", 8), ("quadruped", 4)])
def test_fused_call_equals_composed_path(engine, name, T):
    m, task, mocap, X, U, Tm = tc.batch(name, n=T)
    be = engine(name)
    be.set_task(task)
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    kw = dict(regularization_type=0, action_limits_on=1)
    fused = be.trajectory_ilqg(X, U, Tm, res, mocap=mocap, eps=1e-6, centered=False, **kw)
    fd = be.transition_fd(X, U, Tm, mocap=mocap, eps=1e-6, centered=False, last_is_terminal=True)
    cd = be.cost_derivatives(res, fd["C"], fd["D"], last_is_terminal=True, hessians=True)
    rng = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2).copy()
    rng[np.ravel(m["actuator_ctrllimited"]) == 0] = (-np.inf, np.inf)
    comp = be.ilqg_backward_pass(fd["A"], fd["B"], cd["cx"], cd["cu"], cd["cxx"], cd["cxu"], cd["cuu"], U, rng, **kw)
    assert fused["status"][0] == 1 and list(fused["status"]) == list(comp["status"])
    assert np.array_equal(fused["failure"], fd["failure"])
    for k in rc.OUT_KEYS:
        assert np.isfinite(fused[k]).all(), k
        assert np.array_equal(fused[k], comp[k]), k
    assert np.abs(fused["K"]).max() > 0
    # the C++ ComputeFused is the same call
    nd, nu = fused["Vx"].shape[1], fused["k"].shape[1]
    bp = D.ILQGBackwardPass(nd, nu, T)
    o = bp.compute_fused(be, X, U, Tm, res, mocap=mocap, tol=1e-6, mode=0, **kw)
    for k in rc.OUT_KEYS:
        assert np.array_equal(o[k], fused[k]), k


def test_misuse_is_refused_with_a_message(engine):
    m, task, mocap, X, U, Tm = tc.batch("cartpole", n=3)
    be = engine("cartpole")
    be.set_task(task)
    c = rc.trajectory(4, 1, 3)
    args = [c[k] for k in NAMES]
    with pytest.raises(RuntimeError, match="T < 2"):
        be.ilqg_backward_pass(c["A"], c["B"], c["cx"][:1], c["cu"][:1], c["cxx"][:1], c["cxu"][:1], c["cuu"][:1], c["actions"], c["action_limits"])
    bad = capi.riccati_settings(); bad.struct_size -= 8
    with pytest.raises(RuntimeError, match="struct_size"):
        be.ilqg_backward_pass(*args, settings=bad)
    with pytest.raises(RuntimeError, match="null input"):
        be.ilqg_backward_pass(*args[:7], None, None, action_limits_on=1)          # limits on without actions / limits
    dp = capi.c_double_p
    z = np.zeros(64); reg = np.ones(2); s = capi.riccati_settings()
    p = z.ctypes.data_as(dp)
    assert be.lib.mjpc_hip_ilqg_backward_pass(be.h, 3, 4, 1, None, p, p, p, p, p, p, p, p, C.byref(s), reg.ctypes.data_as(dp), reg[1:].ctypes.data_as(dp),
                                              *([None] * 10), None) == -1
    assert b"null input" in be.lib.mjpc_hip_last_error()
    assert be.lib.mjpc_hip_ilqg_backward_pass(be.h, 3, 0, 1, p, p, p, p, p, p, p, p, p, C.byref(s), reg.ctypes.data_as(dp), reg[1:].ctypes.data_as(dp),
                                              *([None] * 10), None) == -1
    assert b"nd < 1" in be.lib.mjpc_hip_last_error()
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    with pytest.raises(RuntimeError, match="T < 2"):
        be.trajectory_ilqg(X[:1], U[:1], Tm[:1], res[:1])
    with pytest.raises(RuntimeError, match="eps <= 0"):
        be.trajectory_ilqg(X, U, Tm, res, eps=0.0)
    # a plan in flight
    kw = dict(state=X[0], mocap=mocap, time=0.0, knot_times=np.array([0.0, 0.2]), knot_values=np.zeros((2, m["nu"])), interpolation=1, num_trajectory=4,
              horizon=2, sigma=(0.1, 0.0), seed=3)
    inp = be.make_input(**kw)
    be.plan_async(inp)
    with pytest.raises(RuntimeError, match="in flight"):
        be.ilqg_backward_pass(*args)
    with pytest.raises(RuntimeError, match="in flight"):
        be.trajectory_ilqg(X, U, Tm, res)
    be.plan_fetch(inp)
    o = be.ilqg_backward_pass(*args)
    assert list(o["status"]) == [1, -1, 0] and np.isfinite(o["K"]).all()
