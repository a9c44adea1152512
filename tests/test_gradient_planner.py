"""CPU tier of the cost derivatives and the gradient planner's backward recursion: the kernel source (csrc/cost_derivatives.h) in the
1-lane emulation against the numpy mirror (gradient_planner_mirror.py, written from the reference text) and against finite differences
of the cost itself; the host Gradient::Compute; the new symbols.

Emulated cost derivatives against the mirror, every entry of cr, cx, cu, cxx, cxu, cuu relative to max(1, |entry|), over the shapes
and tables of gradient_planner_cases.py, measured on the CPU: 0 everywhere, also for the types that go through pow / exp / cosh /
sinh / log and with the risk transform: emulation and mirror call the same libm in the same order.  Ten times that is still 0, so the
CPU bar of every case is bit-equality (the GPU tier records its own figures for the device's libm).

Finite differences (test_cost_derivatives_match_finite_differences): the cost of a knot under the linearised residual r + C dx + D du,
valued by the ORACLE's norm and the risk formula of cost_value, centre-differenced at h = 1e-4; Gauss-Newton is exact for a linear
residual, so truncation and rounding are the only errors.  Largest deviation of the MIRROR from those differences over the cases of
the test, relative to max(1, |entry|): gradient 6.8e-07, Hessian 1.9e-05 (FD_MEASURED); the bar is 10 x that."""
import math
import os
import subprocess

import numpy as np
import pytest

import emu_cost_derivatives_lib as ec
import gradient_planner_cases as gc
import gradient_planner_mirror as gm
import oracle_lib as ol
from mujoco_mpc_amd import capi, cplanner, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mujoco_mpc_amd", "csrc")

CPU_MEASURED = 0.0                       # see the docstring
CPU_BAR = 10 * CPU_MEASURED
FD_MEASURED = {"gradient": 6.8e-07, "hessian": 1.9e-05}
FD_BAR = {k: 10 * v for k, v in FD_MEASURED.items()}
FD_H = 1e-4
SEED_OF_T = {1: 0, 2: 1, 5: 2}


# ----------------------------------------------------------------------------- emulated kernel against the mirror
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("risk", [0.0, 0.7, -0.7])
@pytest.mark.parametrize("kind", ["exact", "all"])
@pytest.mark.parametrize("name", gc.MODELS)
def test_emulated_cost_derivatives_match_mirror(name, kind, risk, T):
    """last knot terminal (T = 1: a terminal knot alone), Hessians on; the kernel is played tile by tile onto NaN-filled outputs"""
    m, t, d, r, Cm, Dm = gc.case(name, kind, risk, T, seed=SEED_OF_T[T])
    if d["nr"] >= 40:
        dense = [n for n, ty in zip(t["dim_norm_residual"], t["norm"]) if ty in (1, 2)]
        assert max(dense) > 16                                               # a dense term wider than a tile side
    assert 1 in list(t["dim_norm_residual"])                                # a single-row term
    if kind == "all":                                                        # every norm type: in one table, or over the three seeds
        tables = [t] if d["nr"] >= 40 else [gc.case(name, kind, risk, 1, seed=s)[1] for s in SEED_OF_T.values()]
        assert {int(ty) for tt in tables for ty in tt["norm"]} == {-1, 0, 1, 2, 3, 5, 6, 7, 8}
    Dn = Dm.copy(); Dn[T - 1] = np.nan                                       # a terminal knot's D is never read
    got = ec.cost_derivatives(m, t, d["nd"], d["nu"], r, Cm, Dn, last_is_terminal=True, hessians=True)
    ref = gm.cost_derivatives(t, r, Cm, Dm, last_is_terminal=True, hessians=True)
    for k in ("cr", "cx", "cu", "cxx", "cxu", "cuu"):
        assert np.isfinite(got[k]).all(), k                                  # every entry written, none from a poisoned value
        dv = gc.dev(got[k], ref[k])
        print(name, kind, risk, T, k, dv)
        if kind == "exact" and risk == 0.0:
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert dv <= CPU_BAR, (k, dv)
    assert not got["cu"][T - 1].any() and not got["cuu"][T - 1].any() and not got["cxu"][T - 1].any()


@pytest.mark.parametrize("name", gc.MODELS)
def test_emulated_gradients_only_mode(name):
    """hessians = 0 writes cr, cx, cu (here with no terminal knot) and the same bits as the Hessian mode does"""
    m, t, d, r, Cm, Dm = gc.case(name, "all", 0.7, 2, seed=7)
    got = ec.cost_derivatives(m, t, d["nd"], d["nu"], r, Cm, Dm, last_is_terminal=False, hessians=False)
    full = ec.cost_derivatives(m, t, d["nd"], d["nu"], r, Cm, Dm, last_is_terminal=False, hessians=True)
    ref = gm.cost_derivatives(t, r, Cm, Dm, last_is_terminal=False, hessians=False)
    assert set(got) == {"cr", "cx", "cu"}
    for k in got:
        assert np.array_equal(got[k], full[k]) and gc.dev(got[k], ref[k]) <= CPU_BAR
    assert np.abs(got["cu"][1]).min() > 0


def test_norm_guards():
    """L2 at s == 0, the rectifier's p <= 0 branch, kNull, L22's max(c, mjMINVAL) at c = 1e-18, the smooth abs at s == 0"""
    m, task, d, _, _, _ = gc.case("particle", "exact", 0.0, 1)
    for norms, prm, r in (([2, 2], [0.0, 0.0], [0.0, 0.0, 0.0, 0.0]), ([8, 8], [0.0, -1.0], [0.3, -0.2, 0.0, 0.5]), ([-1, -1], [], [0.4, 0.5, 0.6, 0.7]),
                          ([1, 6], [0.1, 1.5, 0.0], [1e-9, 0.0, 0.0, 0.0])):
        t = dict(task)
        t["num_term"] = 2; t["dim_norm_residual"] = np.array([2, 2], np.int32); t["norm"] = np.array(norms, np.int32)
        t["num_norm_parameter"] = np.array([len(gc.PARAMS[n]) for n in norms], np.int32); t["norm_parameter"] = np.array(prm, float)
        t["weight"] = np.array([1.0, 2.0])
        rng = np.random.default_rng(5)
        Cm = rng.standard_normal((1, 4, d["nd"])); Dm = rng.standard_normal((1, 4, d["nu"]))
        got = ec.cost_derivatives(m, t, d["nd"], d["nu"], np.array([r]), Cm, Dm, False, True)
        ref = gm.cost_derivatives(t, np.array([r]), Cm, Dm, False, True)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (norms, k)
        if norms[0] == 2:
            assert not got["cr"].any() and not got["cxx"].any()
        if norms[0] == 8:
            assert list(got["cr"][0]) == [1.0, 0.0, 0.0, 1.0] and not got["cxx"].any()
        if norms[0] == -1:
            assert list(got["cr"][0]) == [1.0, 0.0, 1.0, 0.0] and not got["cuu"].any()


# ----------------------------------------------------------------------------- independent check: finite differences of the cost
def _knot_cost(task, T, x):
    """cost of one knot's residual x by the oracle's norm and cost_value's risk formula, with the per-knot weights weight / T"""
    c = 0.0
    fs = ps = 0
    prm = np.asarray(task["norm_parameter"], float).ravel()
    for i in range(int(task["num_term"])):
        ni, npar = int(task["dim_norm_residual"][i]), int(task["num_norm_parameter"][i])
        c += float(task["weight"][i]) / T * ol.norm(x[fs:fs + ni], list(prm[ps:ps + npar]), int(task["norm"][i]))
        fs += ni; ps += npar
    R = float(task["risk"])
    return c if abs(R) < 1e-6 else (math.exp(R * c) - 1.0) / R


def fd_cost_derivatives(task, r, Cm, Dm, h=FD_H):
    """centre differences in z = (dx, du) of _knot_cost(r + [C | D] z) at z = 0 -> dict(cx, cu, cxx, cxu, cuu).  With risk the
    reference forms its outer products from the gradients it has already scaled by s = exp(risk c), where the derivative of the
    risk-sensitive cost has the unscaled ones: expected = differences + (risk s - risk / s) g g', g and s = 1 + risk * cost from the
    differences' side."""
    T, nr, nd = Cm.shape; nu = Dm.shape[2]; n = nd + nu
    o = dict(cx=np.zeros((T, nd)), cu=np.zeros((T, nu)), cxx=np.zeros((T, nd, nd)), cxu=np.zeros((T, nd, nu)), cuu=np.zeros((T, nu, nu)))
    R = float(task["risk"])
    for t in range(T):
        J = np.concatenate([Cm[t], Dm[t]], axis=1)
        f = lambda z: _knot_cost(task, T, r[t] + J @ z)      # noqa: E731
        e = np.eye(n) * h
        g = np.array([(f(e[i]) - f(-e[i])) / (2 * h) for i in range(n)])
        H = np.zeros((n, n))
        for i in range(n):
            for j in range(i, n):
                H[i, j] = H[j, i] = (f(e[i] + e[j]) - f(e[i] - e[j]) - f(-e[i] + e[j]) + f(-e[i] - e[j])) / (4 * h * h)
        if abs(R) >= 1e-6:
            s = 1.0 + R * f(np.zeros(n))
            H = H + (R * s - R / s) * np.outer(g, g)
        o["cx"][t] = g[:nd]; o["cu"][t] = g[nd:]; o["cxx"][t] = H[:nd, :nd]; o["cxu"][t] = H[:nd, nd:]; o["cuu"][t] = H[nd:, nd:]
    return o


@pytest.mark.parametrize("risk", [0.0, 0.7, -0.7])
@pytest.mark.parametrize("name", ["particle", "cartpole", "filter_arm"])
def test_cost_derivatives_match_finite_differences(name, risk):
    worst = {"gradient": 0.0, "hessian": 0.0}
    for seed in range(3):                      # (the particle's four rows take other norm types with every seed)
        m, t, d, r, Cm, Dm = gc.case(name, "all", risk, 2, seed=seed)
        got = ec.cost_derivatives(m, t, d["nd"], d["nu"], r, Cm, Dm, False, True)
        fd = fd_cost_derivatives(t, r, Cm, Dm)
        for k in fd:
            kk = "gradient" if k in ("cx", "cu") else "hessian"
            worst[kk] = max(worst[kk], gc.dev(got[k], fd[k]))
    print(name, risk, worst)
    assert worst["gradient"] <= FD_BAR["gradient"] and worst["hessian"] <= FD_BAR["hessian"]


# ----------------------------------------------------------------------------- backward recursion
def _lqr():
    """the problem of the reference's gradient test: x' = (x0 + x1, x1 + u), cost 0.5 |x|^2 + 0.5 u^2, n 2, m 1, T 3, u = 0.5"""
    n, m, T = 2, 1, 3

    def rollout(u, x0):
        x = np.zeros((T, n)); x[0] = x0; J = 0.0
        for t in range(T - 1):
            J += 0.5 * x[t] @ x[t] + 0.5 * u[t] @ u[t]
            x[t + 1] = (x[t, 0] + x[t, 1], x[t, 1] + u[t, 0])
        return J + 0.5 * x[T - 1] @ x[T - 1], x
    return n, m, T, rollout


def test_gradient_compute_on_the_lqr_problem():
    n, m, T, rollout = _lqr()
    u = np.full((T - 1, m), 0.5); x0 = np.zeros(n)
    _, x = rollout(u, x0)
    A = np.tile(np.array([[1.0, 1.0], [0.0, 1.0]]), (T, 1, 1)); B = np.tile(np.array([[0.0], [1.0]]), (T, 1, 1))
    cx = x.copy(); cu = np.zeros((T, m)); cu[:T - 1] = u
    o = derivatives.gradient_compute(A, B, cx, cu)
    assert o["status"] == 0
    eps = 1e-6
    for i in range(T - 1):
        up, um = u.copy(), u.copy(); up[i] += eps; um[i] -= eps
        assert abs((rollout(up, x0)[0] - rollout(um, x0)[0]) / (2 * eps) - o["Qu"][i, 0]) < 1e-3
    for i in range(n):
        xp, xm = x0.copy(), x0.copy(); xp[i] += eps; xm[i] -= eps
        assert abs((rollout(u, xp)[0] - rollout(u, xm)[0]) / (2 * eps) - o["Vx"][0, i]) < 1e-3
    assert np.array_equal(o["k"][:T - 1], -o["Qu"]) and np.array_equal(o["k"][T - 1], o["k"][T - 2])
    assert o["dV"][0] == -(o["Qu"][1, 0] * o["Qu"][1, 0]) - (o["Qu"][0, 0] * o["Qu"][0, 0]) and o["dV"][1] == 0


@pytest.mark.parametrize("nd,nu,T", [(4, 2, 3), (11, 4, 2), (36, 12, 5), (54, 21, 4), (9, 1, 6)])
def test_host_gradient_is_bit_equal_to_the_emulated_backward_kernel(nd, nu, T):
    rng = np.random.default_rng(nd * 100 + T)
    A = rng.standard_normal((T - 1, nd, nd)); B = rng.standard_normal((T - 1, nd, nu)); cx = rng.standard_normal((T, nd)); cu = rng.standard_normal((T, nu))
    host = derivatives.gradient_compute(A, B, cx, cu)
    emu = ec.gradient_backward(A, B, cx, cu)
    mir = gm.gradient_backward(A, B, cx, cu)
    for k in ("k", "Vx", "Qx", "Qu", "dV"):
        assert np.isfinite(emu[k]).all()
        assert np.array_equal(host[k], emu[k]) and np.array_equal(mir[k], emu[k]), k
    assert np.abs(emu["Vx"][0]).max() > 0


# ----------------------------------------------------------------------------- the gradient is the return's gradient
RETURN_GRADIENT_MEASURED = gc.RETURN_GRADIENT_MEASURED


def test_mirror_gradient_is_the_oracle_returns_gradient():
    import transition_cases as tc
    import transition_mirror as tm
    m, task, state, kt, knots, H = gc.return_gradient_setup()
    o = ol.Oracle(m, task)
    ostep = tc.oracle_step(m, task, None)

    def plan_all(s, cand):
        return o.plan(s, None, 0.0, kt, knots, 0, len(cand), H, sigma=(0.0, 0.0), candidate_knots=cand)

    def gradient(x, u, t, r):
        A, B, Cm, Dm, fail, _ = tm.Mirror(m, task).fd(ostep, x, u, t, 1e-6, True, last_is_terminal=False)
        assert not fail.any()
        cd = gm.cost_derivatives(task, r, Cm, Dm, True, False)
        bw = gm.gradient_backward(A, B, cd["cx"], cd["cu"])
        return dict(Qu=bw["Qu"], Vx=bw["Vx"], cu_last=gm.cost_derivatives(task, r, Cm, Dm, False, False)["cu"][-1])
    du, dx, _, _ = gc.return_gradient_deviation(plan_all, gradient, state, kt, knots, H)
    print("Qu", du, "Vx[0]", dx)
    assert du <= 10 * RETURN_GRADIENT_MEASURED["Qu"] and dx <= 10 * RETURN_GRADIENT_MEASURED["Vx"]


# ----------------------------------------------------------------------------- symbols, ABI, refusals
def test_new_symbols_exist_and_the_abi_is_unchanged():
    lib = capi.load_engine()
    for sym in ("mjpc_hip_cost_derivatives", "mjpc_hip_trajectory_gradient", "mjpc_cd_create", "mjpc_cd_destroy", "mjpc_cd_reset", "mjpc_cd_compute",
                "mjpc_cd_blocks", "mjpc_gd_gradient_compute"):
        assert hasattr(lib, sym), sym
    assert lib.mjpc_hip_version() == 4
    assert [getattr(lib, "mjpc_hip_sizeof_" + w)() for w in ("model", "task", "plan_input", "plan_output")] == ABI_SIZES


ABI_SIZES = [1152, 136, 160, 104]       # the structs' sizes before the two calls were added


def test_refusals_carry_a_message():
    lib = capi.load_engine()
    z = np.zeros(4).ctypes.data_as(capi.c_double_p)
    assert lib.mjpc_hip_cost_derivatives(None, 2, z, z, z, 1, 1, z, z, z, z, z, z) == -1
    assert b"mjpc_hip_cost_derivatives" in lib.mjpc_hip_last_error()
    assert lib.mjpc_hip_trajectory_gradient(None, 2, z, z, z, z, None, None, 1e-6, 0, z, z, z, z, z, np.zeros(2, np.int32).ctypes.data_as(capi.c_int_p)) == -1
    assert b"mjpc_hip_trajectory_gradient" in lib.mjpc_hip_last_error()
    with pytest.raises(cplanner.PlannerError, match="T < 2"):
        derivatives.gradient_compute(np.zeros((1, 2, 2)), np.zeros((1, 2, 1)), np.zeros((1, 2)), np.zeros((1, 1)))


@pytest.mark.parametrize("tu", ["rollout_cached", "rollout_direct", "rollout_dense2", "rollout_dense2h", "rollout_spill", "rollout_step_cached",
                                "rollout_step_direct", "rollout_step_spill"])
def test_rollout_and_step_translation_units_do_not_reach_the_new_header(tu):
    import __graft_entry__ as g
    deps = subprocess.check_output([g.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-M", os.path.join(CSRC, tu + ".hip")], cwd=CSRC).decode()
    names = {os.path.basename(p) for p in deps.replace("\\\n", " ").split()}
    assert "core.h" in names and "cost_derivatives.h" not in names


# ----------------------------------------------------------------------------- policy, spline mappings, planner (host pieces)
@pytest.mark.parametrize("rep", [0, 1, 2])
def test_spline_mapping_times_parameters_is_the_interpolation(rep):
    """zero_test.cc / linear_test.cc / cubic_test.cc: mapping * parameters equals the interpolated actions, L1 error below 1e-5, at their
    n 2, S 6, T 10; the C++ mapping equals the mirror's"""
    M = cplanner.gradient_spline_mapping(rep, 2, gc.MAP_X, gc.MAP_T)
    want = np.array([gm.interpolate(rep, float(t), gc.MAP_X, gc.MAP_Y) for t in gc.MAP_T])
    assert np.abs(M @ gc.MAP_Y.ravel() - want.ravel()).sum() < 1.0e-5
    big = [[-1e9, 1e9]] * 2
    got = np.array([cplanner.gradient_policy_action(rep, big, gc.MAP_X, gc.MAP_Y, float(t)) for t in gc.MAP_T])
    assert np.abs(M @ gc.MAP_Y.ravel() - got.ravel()).sum() < 1.0e-5
    assert np.array_equal(M, gm.spline_mapping(rep, 2, gc.MAP_X, gc.MAP_T))
    assert M.shape == (20, 12) and np.allclose(M.sum(axis=1), 1.0, atol=1e-12)


# GradientPolicy::Action against the engine's spline (the oracle's restatement of it) at 200 times inside and outside the knots:
# zero and linear are the same arithmetic; whether they are the same bits, and cubic's largest difference, measured on the CPU
SPLINE_MEASURED = {0: 0.0, 1: 0.0, 2: 0.0}


@pytest.mark.parametrize("rep", [0, 1, 2])
def test_policy_action_against_the_engine_spline(rep):
    rng = np.random.default_rng(3)
    times = np.cumsum(rng.uniform(0.05, 0.3, 9)); vals = rng.uniform(-0.8, 0.8, (9, 3))
    cr = [[-1.0, 1.0]] * 3
    worst = 0.0
    for t in np.concatenate([rng.uniform(times[0] - 0.2, times[-1] + 0.2, 200), times]):
        a = cplanner.gradient_policy_action(rep, cr, times, vals, float(t))
        assert np.array_equal(a, gm.policy_action(rep, cr, times, vals, float(t)))          # the C++ policy is the mirror's, bit for bit
        e = np.clip(ol.spline_sample(times, vals, rep, float(t)), -1.0, 1.0)
        worst = max(worst, float(np.abs(a - e).max()))
    print("representation", rep, "largest difference from the engine spline", worst)
    if rep < 2:
        assert worst == SPLINE_MEASURED[rep]
    else:
        assert worst <= 10 * SPLINE_MEASURED[2]
    vals[4] = 5.0                                                                          # clamped to the ctrlrange
    assert cplanner.gradient_policy_action(rep, cr, times, vals, float(times[4])).max() == 1.0


def test_more_than_25_spline_points_is_refused():
    from mujoco_mpc_amd.modelgen import particle
    m, task, d = particle(timestep=0.1)
    p = cplanner.GradientPlanner()
    with pytest.raises(cplanner.PlannerError, match="25"):
        p.Initialize(m, task, dict(gradient_spline_points=26), max_samples=4, max_horizon=30)
    lib = capi.load_engine()
    for sym in ("mjpc_gd_create", "mjpc_gd_optimize_policy", "mjpc_gd_policy", "mjpc_gd_best_trajectory", "mjpc_gd_values", "mjpc_gd_timings",
                "mjpc_gd_spline_mapping", "mjpc_gd_policy_action"):
        assert hasattr(lib, sym), sym


def test_planner_mirror_on_the_oracle_solves_the_reference_particle_task():
    """the mirror of the planner loop over ORACLE rollouts and mirror derivatives over oracle steps, at the reference's GradientPlannerTest
    settings and bars (50 iterations, 26 steps of 0.1 s): step sizes ascend from min to 1 and end in 0, the winner order is the reference's, the
    return never rises, and the particle approaches the goal"""
    import transition_cases as tc
    import transition_mirror as tm
    from mujoco_mpc_amd.modelgen import particle
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    ostep = tc.oracle_step(m, task, mocap)
    mir = tm.Mirror(m, task)

    def derivatives(x, u, t, r):
        A, B, Cm, Dm, fail, _ = mir.fd(ostep, x, u, t, 1e-5, False, last_is_terminal=True)
        cd = gm.cost_derivatives(task, r, Cm, np.nan_to_num(Dm), True, False)
        bw = gm.gradient_backward(np.nan_to_num(A), np.nan_to_num(B), cd["cx"], cd["cu"])
        return dict(k=bw["k"], dV=bw["dV"], failure=fail)
    c = gc.PARTICLE_TEST
    pl = gm.GradientPlannerMirror(m, gc.oracle_plan_all(m, task, mocap), derivatives, c["spline_points"], 1, c["num_trajectory"])
    pl.set_state(d["state"], 0.0)
    best = []
    for it in range(c["iterations"]):
        pl.optimize(c["steps"])
        assert not pl.failed
        best.append(min(pl.returns.min(), best[-1] if best else np.inf))
        assert pl.steps[0] == pytest.approx(1e-8) and pl.steps[-2] == 1.0 and pl.steps[-1] == 0.0 and list(pl.steps[:-1]) == sorted(pl.steps[:-1])
        lower = [j for j in range(c["num_trajectory"]) if pl.returns[j] < pl.returns[-1]]
        if lower:                                                   # the lowest return wins; among equal ones the HIGHEST index (strict <, j descending)
            lo = min(pl.returns[j] for j in lower)
            assert pl.winner == max(j for j in lower if pl.returns[j] == lo)
        else:
            assert pl.winner == c["num_trajectory"] - 1
    assert all(b <= a for a, b in zip(best, best[1:])) and best[-1] < best[0]
    x = pl.best["states"][-1]
    print("final state", x, "goal", mocap[:2])
    assert abs(x[0] - mocap[0]) < 1e-2 and abs(x[1] - mocap[1]) < 1e-2 and abs(x[2]) < 1e-1 and abs(x[3]) < 1e-1
    assert np.abs(pl.best["actions"]).max() <= 1.0
