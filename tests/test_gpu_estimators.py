"""GPU tier of the state estimators: mjpc_hip_unscented_moments against the numpy mirror over the device's own step_batch, chunking,
mjpc_hip_linearize_step against transition_fd and step_batch, the C++ classes (mujoco_mpc_amd/estimators.py) against the mirror filters
and the particle's closed form, and the failure paths.  The stepped sigma rows are bit-equal to step_batch of the mirror's table on every model; models
without a quaternion are bit-equal to the mirror throughout; the quaternion-dependent entries of the sphere and the A1 stay within the
bars measured on the CPU between the emulation and the mirror (tests/estimator_cases.py), never within anything derived from device output."""
import numpy as np
import pytest

import estimator_cases as ec
import estimator_mirror as em
import transition_cases as tc
from estimator_cases import CLOSED_FORM_BAR, KALMAN_COVARIANCE_BAR, MOMENTS_BAR, UPDATE_BAR
from mujoco_mpc_amd import estimators as E
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

MOMENT_KEYS = ("state_mean", "sensor_mean", "cov_ss", "cov_sy", "cov_yy", "sigma_next")


def dev(got, want):
    return float(np.nanmax(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if np.size(got) else 0.0


def backend(c, max_samples=256):
    return HipBackend(c["model"], c["task"], max_samples=max_samples, max_horizon=2)


def step_fn(be, mocap):
    def step(S, U, T):
        o = be.step_batch(S, U, T, mocap=mocap)
        return o["next_states"], o["residual"], o["failure"]
    return step


def moments_inputs(name):
    c = ec.case(name); nd = c["dims"]["nd"]
    return c, em.chol(ec.covariance(name)), em.weights(nd), np.full(nd, 1e-4) * (1 + 0.1 * np.arange(nd)), np.full(c["ns"], 1e-4) * (1 + 0.2 * np.arange(c["ns"]))


def device_moments(be, c, L, w, q, r, **kw):
    return be.unscented_moments(c["state"], L, w["sigma_step"], (w["mean0"], w["cov0"], w["sigma"]), c["ctrl"], c["time"], q, r,
                                sensor_first_row=c["first"], num_sensor=c["ns"], mocap=c["mocap"], **kw)


@pytest.mark.parametrize("name", ec.MODELS)
def test_unscented_moments_match_mirror_over_step_batch(name):
    c, L, w, q, r = moments_inputs(name)
    be = backend(c)
    mir = em.Mirror(c["model"], c["task"], c["first"], c["ns"])
    ref = mir.moments(step_fn(be, c["mocap"]), c["state"], L, w, c["ctrl"], c["time"], q, r)      # sigma_next: step_batch of the mirror's table
    L_in = L + np.triu(np.full_like(L, np.nan), 1)                                               # entries above the diagonal are not read
    out = device_moments(be, c, L_in, w, q, r)
    assert out["failure"] == 0 and ref["failure"] == 0
    # the table is the mirror's bit for bit on every model, so the stepped rows and everything without a quaternion in it are too
    for k in MOMENT_KEYS if name in ec.PLAIN else ("sigma_next", "sensor_mean", "cov_yy"):
        assert np.array_equal(out[k], ref[k]), k
    if name not in ec.PLAIN:
        figures = {k: dev(out[k], ref[k]) for k in MOMENT_KEYS}
        print(name, "moments", figures, "bar", MOMENTS_BAR[name])
        assert max(figures.values()) <= MOMENTS_BAR[name]
        qa = mir.quats[0]
        assert out["state_mean"][qa:qa + 4] @ out["sigma_next"][-1, qa:qa + 4] > 0
    # without the rows handed back the moments are the same; a second call repeats the first bit for bit
    lean = device_moments(be, c, L_in, w, q, r, sigma_next=False)
    again = device_moments(be, c, L_in, w, q, r)
    assert lean["sigma_next"] is None and all(np.array_equal(lean[k], out[k]) for k in MOMENT_KEYS[:-1]) and all(np.array_equal(again[k], out[k]) for k in MOMENT_KEYS)
    be.close()


def test_chunked_moments_equal_one_launch():
    """A1: 73 rows, ten launches of at most 8 workgroups against one launch"""
    c, L, w, q, r = moments_inputs("quadruped")
    outs = []
    for cap in (8, 256):
        be = backend(c, max_samples=cap)
        outs.append(device_moments(be, c, L, w, q, r))
        be.close()
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in MOMENT_KEYS) and outs[0]["failure"] == outs[1]["failure"] == 0


@pytest.mark.parametrize("name", ["particle", "quadruped"])
@pytest.mark.parametrize("centered", [False, True])
def test_linearize_step(name, centered):
    c = ec.case(name)
    be = backend(c)
    x, u, t = c["state"], c["ctrl"], c["time"]
    out = be.linearize_step(x, u, t, mocap=c["mocap"], eps=1e-6, centered=centered)
    fd = be.transition_fd(x[None], u[None], np.array([t]), mocap=c["mocap"], eps=1e-6, centered=centered)
    st = be.step_batch(x[None], u[None], np.array([t]), mocap=c["mocap"])
    assert np.array_equal(out["A"], fd["A"][0]) and np.array_equal(out["C"], fd["C"][0]) and out["failure"] == fd["failure"][0] == 0
    assert np.array_equal(out["next_state"], st["next_states"][0]) and np.array_equal(out["residual"], st["residual"][0])
    assert np.abs(out["A"]).max() > 0.5 and np.abs(out["C"]).max() > 0.5
    be.close()


def run_filters(name, updates, full_covariance=False):
    """the same updates through the two classes and the two mirror filters (over the device's step_batch); yields per update"""
    c = ec.case(name)
    be = backend(c)
    step = step_fn(be, c["mocap"])
    kw = dict(epsilon=1e-6, flg_centered=True)
    dk, du = E.Kalman(be, c["first"], c["ns"], **kw), E.Unscented(be, c["first"], c["ns"], **kw)
    mk = em.Kalman(c["model"], c["task"], step, c["first"], c["ns"], eps=1e-6, centered=True)
    mu = em.Unscented(c["model"], c["task"], step, c["first"], c["ns"])
    for f in (dk, du, mk, mu):
        f.Reset(c["state"], c["time"])
        if full_covariance:
            f.covariance = ec.covariance(name)
        if c["mocap"] is not None and hasattr(f, "SetShared"):
            f.SetShared(mocap=c["mocap"])
    rng = np.random.default_rng(9)
    x = c["state"].copy(); t = c["time"]
    for k in range(updates):
        u = rng.uniform(-0.3, 0.3, c["dims"]["nu"])
        nxt, res, fail = step(x[None], u[None], np.array([t]))
        y = res[0, c["first"]:c["first"] + c["ns"]] + 1e-2 * rng.standard_normal(c["ns"])      # sensors at the truth + noise of variance 1e-4
        status = [f.Update(u, y) for f in (dk, du, mk, mu)]
        yield k, status, dk, du, mk, mu
        x, t = nxt[0], t + c["model"]["timestep"]
    dk.close(); du.close(); be.close()


@pytest.mark.parametrize("name", ["particle", "cartpole"])
def test_classes_match_mirror_over_20_updates(name):
    moved = 0.0
    x0 = ec.case(name)["state"]
    for k, status, dk, du, mk, mu in run_filters(name, 20):
        assert status == [0, 0, 0, 0], (k, status)
        assert np.array_equal(dk.state, mk.state) and np.array_equal(dk.covariance, mk.covariance), k
        assert np.array_equal(du.state, mu.state) and np.array_equal(du.covariance, mu.covariance), k
        assert dk.time == mk.time and du.time == mu.time
        moved = max(moved, float(np.abs(du.state - x0).max()))
        assert np.linalg.eigvalsh(du.covariance).min() > 0
    assert moved > 1e-3


@pytest.mark.parametrize("name", ["filter_arm", "sphere", "quadruped"])
def test_classes_match_mirror_over_one_update(name):
    for k, status, dk, du, mk, mu in run_filters(name, 1, full_covariance=True):
        assert status == [0, 0, 0, 0], status
        if name in ec.PLAIN:
            assert np.array_equal(dk.state, mk.state) and np.array_equal(dk.covariance, mk.covariance)
            assert np.array_equal(du.state, mu.state) and np.array_equal(du.covariance, mu.covariance)
        else:
            # the unscented filter at the bar of the CPU tier's one-update test.  The Kalman filter's state goes through the same
            # quaternion integration and one step as the unscented filter's, so it shares that bar; its covariance may move by what a
            # QUAT_BAR-sized change of A's quaternion rows moves it (test_one_kalman_update_under_the_quaternion_row_bar)
            fu = max(dev(du.state, mu.state), dev(du.covariance, mu.covariance))
            fk = (dev(dk.state, mk.state), dev(dk.covariance, mk.covariance))
            print(name, "one update: unscented", fu, "bar", UPDATE_BAR[name], "kalman state, covariance", fk, "bars", UPDATE_BAR[name], KALMAN_COVARIANCE_BAR[name])
            assert fu <= UPDATE_BAR[name] and fk[0] <= UPDATE_BAR[name] and fk[1] <= KALMAN_COVARIANCE_BAR[name]
        assert abs(du.time - (0.05 + ec.case(name)["model"]["timestep"])) < 1e-15 and np.array_equal(du.covariance, du.covariance.T)


def test_particle_closed_form():
    """both classes against the textbook Kalman filter from the closed-form A, B, C = [I 0], at the CPU tier's bar"""
    m, task, mocap, x0, ctrls, ys, (A, B, Cm) = ec.particle_run()
    be = HipBackend(m, task, max_samples=16, max_horizon=2)
    ekf = E.Kalman(be, 0, 2, epsilon=1e-6, flg_centered=True); ukf = E.Unscented(be, 0, 2)
    for f in (ekf, ukf):
        f.Reset(x0)
        if mocap is not None:
            f.SetShared(mocap=mocap)
    assert np.array_equal(ukf.covariance, 1e-4 * np.eye(4)) and np.all(ukf.noise_process == 1e-4) and np.all(ukf.noise_sensor == 1e-4)
    w = ukf.weights; mw = em.weights(4)
    assert (w["sigma_step"], w["weight_mean0"], w["weight_covariance0"], w["weight_sigma"]) == (mw["sigma_step"], mw["mean0"], mw["cov0"], mw["sigma"])
    x, P = x0.copy(), 1e-4 * np.eye(4)
    worst = {"ekf": 0.0, "ukf": 0.0}
    for k in range(len(ctrls)):
        x, P = em.textbook_kalman(A, B, Cm, 1e-4 * np.eye(4), 1e-4 * np.eye(2), x, P, ctrls[k], ys[k])
        assert ekf.Update(ctrls[k], ys[k]) == E.OK and ukf.Update(ctrls[k], ys[k]) == E.OK
        for key, f in (("ekf", ekf), ("ukf", ukf)):
            worst[key] = max(worst[key], float(np.abs(f.state - x).max()), float(np.abs(f.covariance - P).max()))
    print("particle closed form", worst, "bar", CLOSED_FORM_BAR)
    assert worst["ekf"] <= CLOSED_FORM_BAR and worst["ukf"] <= CLOSED_FORM_BAR
    ekf.close(); ukf.close(); be.close()


def test_failures_are_statuses_and_leave_the_estimate_untouched():
    c = ec.case("quadruped")
    be = backend(c, max_samples=80)
    ukf = E.Unscented(be, c["first"], c["ns"]); ekf = E.Kalman(be, c["first"], c["ns"])
    ukf.SetShared(mocap=c["mocap"]); ekf.SetShared(mocap=c["mocap"])          # (the A1's mocap box left at the origin would sit inside the robot)
    y = np.zeros(c["ns"])
    # a NaN state: every evaluation is a flagged row (MJPC_WARN_BADQPOS), not a fault
    bad = c["state"].copy(); bad[1] = np.nan
    for f in (ukf, ekf):
        f.Reset(bad, 0.25)
        P0 = f.covariance
        assert f.Update(c["ctrl"], y) == E.STEP_FLAGGED and f.last_failure & 1
        assert np.array_equal(f.state, bad, equal_nan=True) and np.array_equal(f.covariance, P0) and f.time == 0.25
    nd = c["dims"]["nd"]
    w = em.weights(nd)
    out = be.unscented_moments(bad, 1e-2 * np.eye(nd), w["sigma_step"], (w["mean0"], w["cov0"], w["sigma"]), c["ctrl"], 0.0, np.zeros(nd), np.zeros(c["ns"]),
                               num_sensor=c["ns"], mocap=c["mocap"])
    assert out["failure"] & 1
    # a covariance that is not positive definite
    ukf.Reset(c["state"], 0.0)
    P = ukf.covariance; P[3, 3] = -1e-4
    ukf.covariance = P
    assert ukf.Update(c["ctrl"], y) == E.COVARIANCE_RANK and np.array_equal(ukf.state, c["state"]) and np.array_equal(ukf.covariance, P) and ukf.time == 0.0
    # a sensor covariance that is not: negative sensor noise far below -C P C'
    ekf.Reset(c["state"], 0.0); ukf.Reset(c["state"], 0.0)
    for f in (ekf, ukf):
        f.noise_sensor = np.full(c["ns"], -1.0)
        P0 = f.covariance
        assert f.Update(c["ctrl"], y) == E.SENSOR_RANK and np.array_equal(f.state, c["state"]) and np.array_equal(f.covariance, P0) and f.time == 0.0
    # after all that a clean update still goes through
    ukf.Reset(c["state"], 0.0)
    nxt = be.step_batch(c["state"][None], c["ctrl"][None], np.zeros(1), mocap=c["mocap"])
    assert ukf.Update(c["ctrl"], nxt["residual"][0, :c["ns"]]) == E.OK and ukf.time == c["model"]["timestep"]
    ukf.close(); ekf.close(); be.close()


def test_misuse_is_refused_with_a_message():
    m, task, mocap, X, U, T = tc.batch("particle_copystate", n=3)
    be = HipBackend(m, task, max_samples=16, max_horizon=4)
    w = em.weights(4)
    args = (X[0], 1e-2 * np.eye(4), w["sigma_step"], (w["mean0"], w["cov0"], w["sigma"]), U[0], 0.0, np.full(4, 1e-4))
    # a row range beyond num_residual (4), ns < 1
    with pytest.raises(RuntimeError, match="outside the task's 4 residual rows"):
        be.unscented_moments(*args, np.full(3, 1e-4), sensor_first_row=2, num_sensor=3, mocap=mocap)
    with pytest.raises(RuntimeError, match="ns < 1"):
        be.unscented_moments(*args, np.zeros(0), sensor_first_row=0, num_sensor=0, mocap=mocap)
    with pytest.raises(ValueError, match="not inside"):
        E.Unscented(be, 3, 2)
    with pytest.raises(RuntimeError, match="eps"):
        be.linearize_step(X[0], U[0], 0.0, mocap=mocap, eps=0.0)
    # a plan in flight: both calls and both classes are refused, and the plan stays fetchable
    kt = np.array([0.0, 0.2]); kv = np.zeros((2, m["nu"]))
    kw = dict(state=X[0], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=1, num_trajectory=4, horizon=4, sigma=(0.1, 0.0), seed=3)
    ref = be.plan(**kw)
    ukf = E.Unscented(be, 0, 2); ekf = E.Kalman(be, 0, 2)
    ukf.Reset(X[0]); ekf.Reset(X[0])
    if mocap is not None:
        ukf.SetShared(mocap=mocap); ekf.SetShared(mocap=mocap)
    inp = be.make_input(**kw)
    be.plan_async(inp)
    with pytest.raises(RuntimeError, match="in flight"):
        be.unscented_moments(*args, np.full(2, 1e-4), num_sensor=2, mocap=mocap)
    with pytest.raises(RuntimeError, match="in flight"):
        be.linearize_step(X[0], U[0], 0.0, mocap=mocap)
    assert ukf.Update(U[0], np.zeros(2)) == E.ENGINE_ERROR and ekf.Update(U[0], np.zeros(2)) == E.ENGINE_ERROR
    assert np.array_equal(ukf.state, X[0]) and np.array_equal(ekf.covariance, 1e-4 * np.eye(4))
    got = be.plan_fetch(inp)
    assert np.array_equal(got["returns"], ref["returns"]) and np.array_equal(got["states"], ref["states"]) and got["winner"] == ref["winner"]
    assert ukf.Update(U[0], X[0, :2]) == E.OK
    ukf.close(); ekf.close(); be.close()
    with pytest.raises(RuntimeError, match="closed"):
        ukf.state
    one = HipBackend(m, task, max_samples=16, max_horizon=1)
    with pytest.raises(RuntimeError, match="max_horizon"):
        one.linearize_step(X[0], U[0], 0.0, mocap=mocap)
    with pytest.raises(RuntimeError, match="max_horizon"):
        one.unscented_moments(*args, np.full(2, 1e-4), num_sensor=2, mocap=mocap)
    one.close()
