"""Shapes, regrouped cost tables and random inputs of the cost-derivative tests (TEST INFRASTRUCTURE ONLY), shared by the CPU tier
(emulation) and the GPU tier.

A model contributes its dimensions (nd + nu: particle 6, cartpole 5, filter_arm 15 with na > 0, the A1 48, the humanoid 75, which is no
multiple of the 16-wide tile) and its residual count; the cost table over those residual rows is regrouped through the task struct:
    exact   types -1, 0, 2, 6 only (products, sums, IEEE sqrt and divide: bit-equal to the mirror at risk 0)
    all     every norm type, the rectifier in both branches (p > 0, p = 0)
Both hold a single-row term, and where the model has the rows (A1, humanoid) a dense-Hessian term of 17 rows: more than a tile side."""
import numpy as np

import transition_cases as tc
import transition_mirror as tm

MODELS = ["particle", "cartpole", "filter_arm", "quadruped", "humanoid_spill"]
PARAMS = {-1: [], 0: [], 1: [0.1, 1.5], 2: [0.1], 3: [0.5], 5: [1.5], 6: [0.1], 7: [0.1, 2.5], 8: [0.3]}


def _table(nr, kind, seed):
    """(dims, norms, params per term) covering nr rows"""
    if kind == "exact":
        cycle = [(-1, 1), (2, 17 if nr >= 40 else 2), (6, 3 if nr >= 40 else 1), (0, 2)]
    else:
        cycle = [(-1, 1), (2, 17 if nr >= 40 else 1), (1, 5 if nr >= 40 else 2), (3, 2), (5, 1), (6, 2), (7, 2), (8, 1), ("8r", 1), (0, 3)]
        if nr < 40:                     # few rows: one or two per term, and the types that do not fit rotate in through the seed (0, 1, 2 cover all)
            k = (3 * seed) % len(cycle)
            cycle = [(t, 1 if t != 1 else 2) for t, _ in cycle[k:] + cycle[:k]]
    dims, norms, prm = [], [], []
    left = nr
    i = 0
    while left > 0:
        ty, n = cycle[i % len(cycle)]
        n = min(n, left)
        if ty == "8r":
            norms.append(8); prm.append([0.0])
        else:
            norms.append(ty); prm.append(PARAMS[ty])
        dims.append(n); left -= n; i += 1
    return dims, norms, prm


def regroup(task, kind, risk, seed=0):
    rng = np.random.default_rng(1000 + seed)
    dims, norms, prm = _table(int(task["num_residual"]), kind, seed)
    t = dict(task)
    t["num_term"] = len(dims)
    t["dim_norm_residual"] = np.array(dims, np.int32); t["norm"] = np.array(norms, np.int32)
    t["num_norm_parameter"] = np.array([len(p) for p in prm], np.int32)
    t["norm_parameter"] = np.array([v for p in prm for v in p], float)
    t["weight"] = rng.uniform(0.2, 2.0, len(dims))
    t["risk"] = float(risk)
    return t


def inputs(nr, nd, nu, T, seed=0):
    """residual entries with 0.1 <= |x| <= 1 (power and smooth-abs-2 losses are singular at 0), Jacobians of unit normals"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 1.0, (T, nr)) * rng.choice([-1.0, 1.0], (T, nr))
    return r, rng.standard_normal((T, nr, nd)), rng.standard_normal((T, nr, nu))


def case(name, kind, risk, T, seed=0):
    m, task, _ = tc.model(name)
    d = tm.dims(m, task)
    t = regroup(task, kind, risk, seed)
    r, Cm, Dm = inputs(d["nr"], d["nd"], d["nu"], T, seed)
    return m, t, d, r, Cm, Dm


def dev(got, want):
    """largest deviation relative to max(1, |entry|); NaN (an entry never written) counts as infinite"""
    if not got.size:
        return 0.0
    e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(np.inf) if np.isnan(e).any() else float(e.max())


# ----------------------------------------------------------------------------- the gradient is the return's gradient
# largest deviation of the mirror over ORACLE steps from centre differences of the oracle's returns (cartpole, H 8, seven zero-order
# knots; relative to max(1, |difference|)), measured on the CPU (tests/test_gradient_planner.py); the GPU tier holds the engine to
# 10 x these.  The reference's own bar for this check is 1e-3.
RETURN_GRADIENT_MEASURED = {"Qu": 9.5e-11, "Vx": 2.9e-07}


def return_gradient_setup():
    """cartpole, H = 8, seven zero-order knots at the step times, controls well inside the ctrlrange, a state off the default one"""
    m, task, d = tc.model("cartpole")
    H, P = 8, 7
    rng = np.random.default_rng(11)
    knots = rng.uniform(-0.3, 0.3, (P, m["nu"]))
    state = np.asarray(d["state"], float) + 0.1 * rng.standard_normal(len(d["state"]))
    return m, task, state, 0.0 + m["timestep"] * np.arange(P), knots, H


def return_gradient_deviation(plan_all, gradient, state, knot_times, knots, H, delta=1e-4):
    """plan_all(state, candidates [N, P, nu]) -> dict(returns [N], states / actions / times / residual [N, H, .]) of explicit zero-order
    candidates; gradient(x, u, time, residual) -> dict(Qu [T-1, nu], Vx [T, nd], cu_last [nu]: cu of the last knot WITH its D).
    Centre differences of the return over every knot and over the initial state against Qu and Vx[0], relative to max(1, |entry|).
    Knot T - 2 is held over the terminal row, whose direct dependence on the action the recursion drops (as the reference does): the
    comparison there is with Qu[T-2] + cu[T-1]."""
    P, nu = knots.shape
    cand = [knots]
    for t in range(P):
        for k in range(nu):
            for s in (1.0, -1.0):
                c = knots.copy(); c[t, k] += s * delta; cand.append(c)
    o = plan_all(state, np.array(cand))
    g = gradient(o["states"][0], o["actions"][0], o["times"][0], o["residual"][0])
    R = o["returns"][1:].reshape(P, nu, 2)
    fd_u = (R[:, :, 0] - R[:, :, 1]) / (2 * delta)
    want = g["Qu"].copy(); want[H - 2] = want[H - 2] + g["cu_last"]
    dev_u = np.abs(fd_u - want) / np.maximum(1.0, np.abs(fd_u))
    fd_x = np.zeros(len(state))
    for i in range(len(state)):                  # (cartpole: slide and hinge, the tangent is the coordinate)
        sp, sm = state.copy(), state.copy(); sp[i] += delta; sm[i] -= delta
        fd_x[i] = (plan_all(sp, knots[None])["returns"][0] - plan_all(sm, knots[None])["returns"][0]) / (2 * delta)
    dev_x = np.abs(fd_x - g["Vx"][0]) / np.maximum(1.0, np.abs(fd_x))
    assert np.abs(fd_u).min() > 1e-6 and np.abs(fd_x).max() > 1e-3          # there is a gradient to compare
    return float(dev_u.max()), float(dev_x.max()), fd_u, want


# ----------------------------------------------------------------------------- the reference's spline-mapping and particle tests
MAP_X = [0.1, 0.3, 0.7, 1.2, 1.21, 1.6]                   # zero_test.cc / linear_test.cc / cubic_test.cc: S 6, n 2, T 10
MAP_Y = np.array([-1.0, 0.2, 0.5, 0.7, 0.1, 0.34, -0.7, 0.9, 0.2, 0.1, -0.05, 1.0]).reshape(6, 2)
MAP_T = MAP_X[0] + (MAP_X[-1] - MAP_X[0]) / 9 * np.arange(10)
PARTICLE_TEST = dict(iterations=50, steps=26, timestep=0.1, spline_points=11, num_trajectory=32)      # gradient_planner_test.cc


def oracle_plan_all(m, task, mocap):
    import oracle_lib as ol
    o = ol.Oracle(m, task)

    def plan_all(state, time, knot_times, cand, rep, H):
        return o.plan(state, mocap, time, knot_times, cand[0], rep, len(cand), H, sigma=(0.0, 0.0), candidate_knots=cand)
    return plan_all
