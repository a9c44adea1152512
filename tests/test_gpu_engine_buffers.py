"""GPU tier of the engine's host-side buffers: one long-lived engine runs a sequence of calls that makes every buffer grown on demand
(noise, knots, candidate table, packed result, the scratch of every one-step call and of the feedback rollouts) grow, then serves smaller
requests out of the larger allocation, and every call's complete output is bit for bit that of the same call on a fresh engine with the
same limits."""
import numpy as np
import pytest

import transition_cases as tc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

MAX_SAMPLES, MAX_HORIZON = 32, 8
USERDATA = np.array([0.25, -1.5, 3.0])


def _model(name):
    """particle: the generic kernel; quadruped: compile-time nv, cached flavour, mocap; three userdata numbers (no residual reads them)
    put the userdata staging to use"""
    m, task, d = tc.model(name)
    if name == "quadruped":
        m = dict(m); m["nuserdata"] = USERDATA.size
    return m, task, d


def _calls(name, m, task, d):
    """the sequence: (name, function of a backend -> dict of arrays / scalars)"""
    nu = m["nu"]
    rng = np.random.default_rng(11)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    ud = USERDATA if m["nuserdata"] else None

    def common(N, P, H):
        return dict(state=d["state"], mocap=mocap, userdata=ud, time=0.0, knot_times=np.linspace(0.0, 0.02 * P, P),
                    knot_values=0.1 * rng.standard_normal((P, nu)), interpolation=1, num_trajectory=N, horizon=H, seed=7, stream=3)

    kw1, kw2, kw3, kw4 = common(4, 2, 4), common(32, 5, 8), common(8, 3, 6), common(8, 3, 6)
    kw2["candidate_knots"] = 0.2 * rng.standard_normal((32, 5, nu))
    cand4 = 0.2 * rng.standard_normal((8, 3, nu)); std4 = np.full(3 * nu, 0.05)
    slot = np.array([1, 3, 2, 7, 1], np.int32); scale = rng.standard_normal(slot.size)
    _, _, _, X, U, T = tc.batch(name, n=40, seed=5)
    X3, U3, T3 = X[:3], U[:3], T[:3]

    def with_all(out, be, N, H, P):
        out = {k: v for k, v in out.items() if not k.endswith("_time_us")}
        out.update({"all_" + k: v for k, v in be.fetch_all(N, H, P).items()})
        return out

    def plain(be):
        return with_all(be.plan(sigma=(0.1, 0.0), **kw1), be, 4, 4, 2)

    def explicit(be):
        return with_all(be.plan(sigma=(0.0, 0.0), **kw2), be, 32, 8, 5)

    def summary(be):
        be.set_fetch_mode(True)
        out = with_all(be.plan(sigma=(0.1, 0.0), **kw3), be, 8, 6, 3)
        out.update({"cand_" + k: v for k, v in be.candidate(out["winner"], 6, 3).items()})
        return out

    def mixed(be):
        be.set_fetch_mode(False)
        out = with_all(be.plan_mixed(4, sigma=(0.0, 0.0), noise_std=std4, nominal_index=0, candidate_knots=cand4, **kw4), be, 8, 6, 3)
        out["gradient"] = be.sample_gradient(slot, scale)
        return out

    def steps(be):
        return be.step_batch(X, U, T, mocap=mocap, userdata=ud)

    def fd(be):
        return be.transition_fd(X3, U3, T3, mocap=mocap, userdata=ud, eps=1e-6)

    # the other calls that lay their scratch out in the one-step and feedback buffers (csrc/carve.h): each at a larger shape first and at a
    # smaller one later, so that the second is served out of an allocation another layout has grown and written
    nq, nv, na, nr = m["nq"], m["nv"], m["na"], task["num_residual"]
    nd = 2 * nv + na
    X6, U6, T6 = X[:6], U[:6], T[:6]
    res6 = 0.1 * rng.standard_normal((6, nr)); C6 = rng.standard_normal((6, nr, nd)); D6 = rng.standard_normal((6, nr, nu))
    factor = 1e-2 * (np.eye(nd) + 0.1 * np.tril(rng.standard_normal((nd, nd))))
    weights = (0.1, 0.2, 0.45 / nd); q = np.full(nd, 1e-4); r = 1e-4 * (1 + 0.2 * np.arange(nr))
    gain = 0.05 * rng.standard_normal((6, nu, nd)); impr = 0.1 * rng.standard_normal((6, nu)); ptimes = 0.01 * np.arange(6)
    alpha = np.linspace(0.0, 1.0, 8); fscale = np.linspace(1.0, 0.3, 8)

    def known(out):
        return {k: v for k, v in out.items() if v is not None}

    def ukf(ns, sigma_next):
        return lambda be: known(be.unscented_moments(X[1], factor, 1.0, weights, U[1], T[1], q, r[:ns], num_sensor=ns, mocap=mocap, userdata=ud,
                                                     sigma_next=sigma_next))

    def lin(centered):
        return lambda be: be.linearize_step(X[2], U[2], T[2], mocap=mocap, userdata=ud, centered=centered)

    def cd(n, hessians):
        return lambda be: be.cost_derivatives(res6[:n], C6[:n], D6[:n], last_is_terminal=True, hessians=hessians, fill=7.0)

    def grad(n, centered):
        return lambda be: be.trajectory_gradient(X6[:n], U6[:n], T6[:n], res6[:n], mocap=mocap, userdata=ud, centered=centered)

    def riccati(n, a, b, limits):
        """the backward pass at its own dimensions a x b: a = 80, b = 10 keeps the kernel's work image out of LDS, behind the block"""
        g = np.random.default_rng(100 * a + b)
        A = np.eye(a) + 0.1 * g.standard_normal((n - 1, a, a)); B = g.standard_normal((n - 1, a, b))
        cxx = np.tile(np.eye(a), (n, 1, 1)); cuu = np.tile(np.eye(b), (n, 1, 1)); cxu = 0.01 * g.standard_normal((n, a, b))
        cx = g.standard_normal((n, a)); cu = g.standard_normal((n, b)); act = 0.1 * g.standard_normal((n, b)); lim = np.tile([-1.0, 1.0], (b, 1))
        return lambda be: be.ilqg_backward_pass(A, B, cx, cu, cxx, cxu, cuu, actions=act if limits else None, action_limits=lim if limits else None,
                                                action_limits_on=limits)

    def ilqg(n, centered):
        return lambda be: be.trajectory_ilqg(X6[:n], U6[:n], T6[:n], res6[:n], mocap=mocap, userdata=ud, centered=centered)

    def feedback(n, H, N, mode, improvement):
        def call(be):
            out = be.plan_feedback(d["state"], 0.0, H, ptimes[:n], X6[:n], U6[:n], gain[:n], alpha[:N], fscale[:N],
                                   action_improvement=impr[:n] if improvement else None, mode=mode, mocap=mocap, userdata=ud)
            return with_all(out, be, N, H, 0)
        return call

    carved = [("unscented_moments", ukf(nr, True)), ("linearize_step", lin(True)), ("cost_derivatives hessians", cd(6, True)),
              ("trajectory_gradient", grad(6, True)), ("ilqg_backward_pass out of LDS", riccati(3, 80, 10, True)), ("trajectory_ilqg", ilqg(6, True)),
              ("plan_feedback time", feedback(4, 6, 8, capi.FEEDBACK_TIME, True)), ("plan_feedback indexed", feedback(6, 6, 8, capi.FEEDBACK_INDEXED, True)),
              ("trajectory_ilqg small", ilqg(2, False)), ("ilqg_backward_pass small", riccati(2, 3, 1, False)), ("trajectory_gradient small", grad(2, False)),
              ("cost_derivatives small", cd(3, False)), ("linearize_step small", lin(False)), ("unscented_moments small", ukf(1, False)),
              ("plan_feedback indexed small", feedback(3, 3, 2, capi.FEEDBACK_INDEXED, False)),
              ("plan_feedback time small", feedback(2, 4, 3, capi.FEEDBACK_TIME, False)), ("step_batch again", steps)]
    return [("plain", plain), ("explicit", explicit), ("summary", summary), ("mixed", mixed), ("step_batch", steps), ("transition_fd", fd),
            ("plain again", plain)] + carved


def _same(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]


@pytest.mark.parametrize("name", ["particle", "quadruped"])
def test_a_long_lived_engine_answers_like_a_fresh_one(name):
    m, task, d = _model(name)
    calls = _calls(name, m, task, d)
    old = HipBackend(m, task, max_samples=MAX_SAMPLES, max_horizon=MAX_HORIZON)
    got = []
    for what, call in calls:
        got.append(call(old))
        fresh = HipBackend(m, task, max_samples=MAX_SAMPLES, max_horizon=MAX_HORIZON)
        want = call(fresh)
        fresh.close()
        assert _same(got[-1], want) == [], (what, _same(got[-1], want))
    assert not old.dense_tier()[1]                 # (below the CU count: the dense tier is not taken)
    old.close()
    assert _same(got[6], got[0]) == []
    # the calls are not trivially equal: different plans gave different winners' rows, the steps moved every row
    assert got[0]["all_states"].shape == (4, 4, got[0]["states"].shape[1]) and np.ptp(got[0]["returns"]) > 0
    assert np.ptp(got[1]["returns"]) > 0 and np.array_equal(got[2]["cand_states"], got[2]["all_states"][got[2]["winner"]])
    assert not got[2]["states"].any() and got[3]["gradient"].any()
    assert got[4]["next_states"].shape[0] == 40 > MAX_SAMPLES and len({r.tobytes() for r in got[4]["next_states"]}) == 40
    assert np.abs(got[5]["A"]).max() > 0.5
    # nor are the carved calls: every block that comes back holds numbers, the filled Hessians are absent without Hessians, the feedback
    # candidates differ, and the steps behind all of them are the steps before all of them
    by = {what: g for (what, _), g in zip(calls, got)}
    assert by["unscented_moments"]["sigma_next"].shape[0] == 2 * by["unscented_moments"]["cov_ss"].shape[0] + 1
    assert "sigma_next" not in by["unscented_moments small"] and by["unscented_moments small"]["cov_yy"].shape == (1, 1)
    assert all(np.abs(by[w]["cov_sy"]).max() > 0 for w in ("unscented_moments", "unscented_moments small"))
    assert all(np.abs(by[w]["A"]).max() > 0.5 for w in ("linearize_step", "linearize_step small"))
    assert np.abs(by["cost_derivatives hessians"]["cxx"]).max() > 0 and "cxx" not in by["cost_derivatives small"]
    assert all(np.abs(by[w]["cx"]).max() > 0 for w in ("cost_derivatives hessians", "cost_derivatives small"))
    assert all(np.abs(by[w]["Vx"]).max() > 0 for w in ("trajectory_gradient", "trajectory_gradient small", "trajectory_ilqg", "trajectory_ilqg small"))
    assert all(np.abs(by[w]["K"]).max() > 0 for w in ("ilqg_backward_pass out of LDS", "ilqg_backward_pass small"))
    assert all(np.ptp(by[w]["returns"]) > 0 for w in ("plan_feedback time", "plan_feedback indexed"))
    assert _same(by["step_batch again"], got[4]) == []
