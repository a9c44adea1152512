"""GPU tier of the cost derivatives (mjpc_hip_cost_derivatives) and the gradient planner's device iteration
(mjpc_hip_trajectory_gradient): the kernel against the numpy mirror at the shapes and tables of the CPU tier, the fused call against the
composed path, a NaN state, misuse, and the C++ CostDerivatives through its C view.

Kernel against the mirror, every entry of cr, cx, cu, cxx, cxu, cuu relative to max(1, |entry|), measured on an MI355X:
    types -1, 0, 2, 6 at risk 0                        bit-equal (asserted as such)
    the same types with risk (device exp)              GPU_MEASURED[model]["exact+risk"]: 3.2e-16 (particle) .. 1.1e-14 (humanoid)
    every type (device pow / exp / cosh / sinh / log)  GPU_MEASURED[model]["all"]: 4.9e-16 (particle) .. 6.1e-14 (humanoid)
(on the CPU the emulation is bit-equal to the mirror in all three, tests/test_gradient_planner.py).  The bar is 10 x the measured figure."""
import numpy as np
import pytest

import gradient_planner_cases as gc
import gradient_planner_mirror as gm
import transition_cases as tc
import transition_mirror as tm
from mujoco_mpc_amd import capi, derivatives
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

GPU_MEASURED = {"particle": {"exact+risk": 3.2e-16, "all": 4.9e-16}, "cartpole": {"exact+risk": 3.2e-16, "all": 4.9e-16},
                "filter_arm": {"exact+risk": 6.2e-16, "all": 6.5e-15}, "quadruped": {"exact+risk": 1.8e-15, "all": 6.1e-15},
                "humanoid_spill": {"exact+risk": 1.1e-14, "all": 6.1e-14}}
GPU_BAR = {n: {k: 10 * v for k, v in d.items()} for n, d in GPU_MEASURED.items()}
SEED_OF_T = {1: 0, 2: 1, 5: 2}
RISKS = (0.0, 0.7, -0.7)

_engines = {}


def _capacity_task(task, tables):
    """a table no smaller than any of `tables` in terms and parameters: the engine is created with it, set_task installs the others"""
    nt = max(int(t["num_term"]) for t in tables + [task])
    nr = int(task["num_residual"])
    dims = [nr // nt + (1 if k < nr % nt else 0) for k in range(nt)]
    t = dict(task)
    t["num_term"] = nt; t["dim_norm_residual"] = np.array(dims, np.int32); t["norm"] = np.full(nt, 7, np.int32)
    t["num_norm_parameter"] = np.full(nt, 2, np.int32); t["norm_parameter"] = np.tile([0.1, 2.5], nt); t["weight"] = np.ones(nt)
    return t


def _tables(name):
    return {(kind, risk, T): gc.case(name, kind, risk, T, seed=SEED_OF_T[T]) for kind in ("exact", "all") for risk in RISKS for T in (1, 2, 5)}


@pytest.fixture(scope="module")
def engine():
    """one engine per model for the whole module (created with a table large enough for every regrouped one)"""
    def get(name):
        if name not in _engines:
            m, task, _ = tc.model(name)
            _engines[name] = HipBackend(m, _capacity_task(task, [c[1] for c in _tables(name).values()]), max_samples=256, max_horizon=2)
        return _engines[name]
    yield get
    for be in _engines.values():
        be.close()
    _engines.clear()


@pytest.mark.parametrize("kind", ["exact", "all"])
@pytest.mark.parametrize("name", gc.MODELS)
def test_cost_derivatives_match_mirror(engine, name, kind):
    be = engine(name)
    worst = {"exact+risk": 0.0, "all": 0.0}
    for (knd, risk, T), (m, t, d, r, Cm, Dm) in _tables(name).items():
        if knd != kind:
            continue
        be.set_task(t)
        Dn = Dm.copy(); Dn[T - 1] = np.nan                                   # a terminal knot's D is never read
        got = be.cost_derivatives(r, Cm, Dn, last_is_terminal=True, hessians=True, fill=np.nan)
        ref = gm.cost_derivatives(t, r, Cm, Dm, last_is_terminal=True, hessians=True)
        for k in ("cr", "cx", "cu", "cxx", "cxu", "cuu"):
            assert np.isfinite(got[k]).all(), (risk, T, k)                   # every entry written
            if kind == "exact" and risk == 0.0:
                assert np.array_equal(got[k], ref[k]), (T, k)
            else:
                key = "all" if kind == "all" else "exact+risk"
                worst[key] = max(worst[key], gc.dev(got[k], ref[k]))
        assert not got["cu"][T - 1].any() and not got["cuu"][T - 1].any() and not got["cxu"][T - 1].any()
    print(name, kind, "largest deviation from the mirror", worst)
    for key, v in worst.items():
        assert v <= GPU_BAR[name][key], (key, v)


@pytest.mark.parametrize("name", ["cartpole", "humanoid_spill"])
def test_gradients_only_mode_and_null_outputs(engine, name):
    be = engine(name)
    m, t, d, r, Cm, Dm = gc.case(name, "all", 0.7, 2, seed=7)
    be.set_task(t)
    full = be.cost_derivatives(r, Cm, Dm, last_is_terminal=False, hessians=True, fill=np.nan)
    got = be.cost_derivatives(r, Cm, Dm, last_is_terminal=False, hessians=False, fill=np.nan)
    assert set(got) == {"cr", "cx", "cu"}
    for k in got:
        assert np.array_equal(got[k], full[k])
    # any output may be NULL: cx alone
    cx = np.full((2, d["nd"]), np.nan)
    dp = capi.c_double_p
    rc = be.lib.mjpc_hip_cost_derivatives(be.h, 2, r.ctypes.data_as(dp), Cm.ctypes.data_as(dp), Dm.ctypes.data_as(dp), 0, 1, None, cx.ctypes.data_as(dp),
                                          None, None, None, None)
    assert rc == 0 and np.array_equal(cx, full["cx"])
    # the C++ class through its C view: the last knot terminal
    cd = derivatives.CostDerivatives(dims=(d["nd"], d["nu"], d["nr"]), T=2)
    o = cd.compute(be, r, Cm, Dm)
    term = be.cost_derivatives(r, Cm, Dm, last_is_terminal=True, hessians=True)
    for k in term:
        assert np.array_equal(o[k], term[k]), k
    cd.close()


FUSED = [("cartpole", 8), ("quadruped", 5), ("filter_arm", 4), ("humanoid_spill", 3)]


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("name,T", FUSED)
def test_fused_gradient_is_bit_equal_to_the_composed_path(engine, name, T, centered):
    """transition_fd, then cost_derivatives(hessians = 0), then the host Gradient::Compute, against one mjpc_hip_trajectory_gradient; the
    task is the model's own"""
    m, task, mocap, X, U, Tm = tc.batch(name, n=T)
    be = engine(name)
    be.set_task(task)
    assert (be.spill_bytes() > 0) == (name == "humanoid_spill")
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    eps = 1e-6
    fd = be.transition_fd(X, U, Tm, mocap=mocap, eps=eps, centered=centered, last_is_terminal=True)
    cd = be.cost_derivatives(res, fd["C"], fd["D"], last_is_terminal=True, hessians=False)
    host = derivatives.gradient_compute(fd["A"], fd["B"], cd["cx"], cd["cu"])
    fused = be.trajectory_gradient(X, U, Tm, res, mocap=mocap, eps=eps, centered=centered)
    for k in ("k", "Vx", "Qx", "Qu", "dV"):
        assert np.isfinite(fused[k]).all() and np.array_equal(fused[k], host[k]), k
    assert np.array_equal(fused["failure"], fd["failure"]) and not fused["failure"].any()
    assert np.abs(fused["Qu"]).max() > 0 and np.abs(fused["Vx"][0]).max() > 0
    assert np.array_equal(fused["k"][T - 1], fused["k"][T - 2]) and np.array_equal(fused["Vx"][T - 1], cd["cx"][T - 1])
    again = be.trajectory_gradient(X, U, Tm, res, mocap=mocap, eps=eps, centered=centered)
    assert all(np.array_equal(fused[k], again[k]) for k in fused)


def test_gradient_is_the_returns_gradient():
    """Qu and Vx[0] of mjpc_hip_trajectory_gradient against centre differences of the engine's own returns; all perturbed policies of the
    knots go in one explicit-candidate plan.  Bars: 10 x what the mirror over oracle steps shows for the same check on the CPU
    (tests/test_gradient_planner.py: Qu 9.5e-11, Vx 2.9e-07)."""
    RETURN_GRADIENT_MEASURED = gc.RETURN_GRADIENT_MEASURED
    m, task, state, kt, knots, H = gc.return_gradient_setup()
    be = HipBackend(m, task, max_samples=64, max_horizon=H)
    P = len(kt)

    def plan_all(s, cand):
        N = len(cand)
        o = be.plan(state=s, mocap=None, time=0.0, knot_times=kt, knot_values=knots, interpolation=0, num_trajectory=N, horizon=H, sigma=(0.0, 0.0),
                    candidate_knots=cand)
        allc = be.fetch_all(N, H, P)
        allc["returns"] = o["returns"]
        return allc

    def gradient(x, u, t, r):
        g = be.trajectory_gradient(x, u, t, r, eps=1e-6, centered=True)
        assert not g["failure"].any()
        fd = be.transition_fd(x, u, t, eps=1e-6, centered=True, last_is_terminal=False)
        g["cu_last"] = be.cost_derivatives(r, fd["C"], fd["D"], last_is_terminal=False, hessians=False)["cu"][-1]
        return g
    du, dx, _, _ = gc.return_gradient_deviation(plan_all, gradient, state, kt, knots, H)
    print("Qu", du, "Vx[0]", dx)
    be.close()
    assert du <= 10 * RETURN_GRADIENT_MEASURED["Qu"] and dx <= 10 * RETURN_GRADIENT_MEASURED["Vx"]


def test_nan_state_sets_that_knots_failure(engine):
    m, task, mocap, X, U, Tm = tc.batch("cartpole", n=4)
    be = engine("cartpole")
    be.set_task(task)
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    Xb = X.copy(); Xb[2, 1] = np.nan
    o = be.trajectory_gradient(Xb, U, Tm, res, mocap=mocap)
    assert o["failure"][2] & 1 and not o["failure"][[0, 1, 3]].any()


def test_misuse_is_refused_with_a_message(engine):
    m, task, mocap, X, U, Tm = tc.batch("cartpole", n=3)
    be = engine("cartpole")
    be.set_task(task)
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    with pytest.raises(RuntimeError, match="T < 2"):
        be.trajectory_gradient(X[:1], U[:1], Tm[:1], res[:1])
    with pytest.raises(RuntimeError, match="eps <= 0"):
        be.trajectory_gradient(X, U, Tm, res, eps=0.0)
    dp = capi.c_double_p
    z = np.zeros(64)
    assert be.lib.mjpc_hip_cost_derivatives(be.h, 0, z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, 1, None, None, None, None, None, None) == -1
    assert b"T < 1" in be.lib.mjpc_hip_last_error()
    assert be.lib.mjpc_hip_cost_derivatives(be.h, 2, None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, 1, None, None, None, None, None, None) == -1
    assert b"null input" in be.lib.mjpc_hip_last_error()
    fail = np.zeros(3, np.int32).ctypes.data_as(capi.c_int_p)
    assert be.lib.mjpc_hip_trajectory_gradient(be.h, 3, None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp), None, None, 1e-6, 0,
                                               None, None, None, None, None, fail) == -1
    assert b"null input" in be.lib.mjpc_hip_last_error()
    # a plan in flight
    kw = dict(state=X[0], mocap=mocap, time=0.0, knot_times=np.array([0.0, 0.2]), knot_values=np.zeros((2, m["nu"])), interpolation=1, num_trajectory=4,
              horizon=2, sigma=(0.1, 0.0), seed=3)
    inp = be.make_input(**kw)
    be.plan_async(inp)
    with pytest.raises(RuntimeError, match="in flight"):
        be.trajectory_gradient(X, U, Tm, res)
    with pytest.raises(RuntimeError, match="in flight"):
        be.cost_derivatives(res, np.zeros((3, 4, 4)), np.zeros((3, 4, 1)))
    be.plan_fetch(inp)
    assert np.isfinite(be.trajectory_gradient(X, U, Tm, res)["Qu"]).all()
