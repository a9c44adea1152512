"""GPU tier of the engine's host-side buffers: one long-lived engine runs a sequence of calls that makes every buffer grown on demand
(noise, knots, candidate table, packed result, the step / finite-difference tables) grow, then serves smaller requests out of the larger
allocation, and every call's complete output is bit for bit that of the same call on a fresh engine with the same limits."""
import numpy as np
import pytest

import transition_cases as tc
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

    return [("plain", plain), ("explicit", explicit), ("summary", summary), ("mixed", mixed), ("step_batch", steps), ("transition_fd", fd),
            ("plain again", plain)]


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
