"""GPU tier of the late residual rows (csrc/late_rows.h): the CPU tier's cases (tests/test_late_rows.py) through HipBackend.step_batch with
the bars measured there between the emulation and the references (tests/late_cases.py; none derived from device output), the A1's touch
rows on the spill and the direct flavour, the estimator calls on the particle that carries an accelerometer, the rows mjpc_hip_plan
writes, and the unchanged step of a table without late blocks."""
import ctypes as C

import numpy as np
import pytest

import emu_late_rows_lib as el
import estimator_cases as ec
import estimator_mirror as em
import late_cases as lc
import late_checks as ck
from mujoco_mpc_amd import estimators as E
from mujoco_mpc_amd.planner import HipBackend
from test_late_rows import _mixed_tables, closed_form_deviation, particle_imu_run

pytestmark = pytest.mark.gpu


def device_step(c, task=None):
    be = HipBackend(c["model"], task or c["task"], max_samples=16, max_horizon=2)
    o = be.step_batch(c["X"], c["U"], c["T"], mocap=c["mocap"])
    n = C.c_int(0)
    spill = be.lib.mjpc_hip_debug_spill(be.h, C.byref(n)) == 1
    be.close()
    return o["next_states"], o["residual"], o["failure"], spill


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", lc.KINEMATIC)
def test_kinematic_rows_against_autodiff(name):
    c = lc.kinematic(name)
    nxt, res, fail, _ = device_step(c)
    assert res.shape[0] == 8 and not fail.any() and np.isfinite(res).all()
    worst, dq, R = ck.kinematic_deviation(c, res)
    print(name, "late rows against the autodiff reference", worst, "bar", lc.KIN_BAR[name], "| qacc against M^-1 (f - c)", dq, "bar", lc.QACC_BAR[name])
    assert worst <= lc.KIN_BAR[name] and dq <= lc.QACC_BAR[name]
    if name == "particle_imu":                                    # at rest: Rᵀ (0, 0, 9.81), bit for bit
        assert np.array_equal(res[0, c["rows"]["accelerometer"]], np.array([0.0, 9.81, 0.0]))


# ------------------------------------------------------------------------------------------------ (b), (c)
def check_touch(name, res, fail):
    c = lc.touch(name); nv = c["nv"]
    assert not fail.any()
    worst, refs = ck.touch_deviation(c, res)
    print(name, "touch rows against the reference, relative to max(1, |force|)", worst, "bar", lc.TOUCH_BAR[name])
    assert worst <= lc.TOUCH_BAR[name]
    if name.startswith("twoball"):
        assert res.shape[0] == 4
        ck.touch_coverage(refs)
        for i, r in enumerate(refs):
            one, both = res[i, nv], res[i, nv + 1]
            assert 0 < one < both and abs(both - r["forces"].sum()) <= lc.TOUCH_BAR[name] * max(1.0, both) and res[i, nv + 2] == 0.0
    else:
        assert res.shape[0] == 6
        ck.touch_coverage(refs, airborne=[(0, 0), (0, 4)])
        assert res[0, nv] == 0.0 and res[0, nv + 4] == 0.0                                     # the foot in the air reads exactly 0
        assert all((res[i, nv:nv + 4] > 0).tolist() == [len(z) > 0 for z in r["included"][:4]] for i, r in enumerate(refs))


@pytest.mark.parametrize("name", lc.TOUCH)
def test_touch_against_the_force_law(name):
    nxt, res, fail, _ = device_step(lc.touch(name))
    check_touch(name, res, fail)


@pytest.mark.parametrize("knob,value", [("spill", "all"), ("no_model_cache", "1")])
def test_a1_touch_on_the_spill_and_direct_flavours(debug_knobs, knob, value):
    """the engine forced onto the flavour that keeps contacts and efc_force in the HBM slab, and onto the one that reads the tables from
    HBM: the late phase reads both through Ctx's accessors"""
    debug_knobs(knob, value)
    nxt, res, fail, spill = device_step(lc.touch("quadruped_elliptic"))
    assert spill == (knob == "spill")
    check_touch("quadruped_elliptic", res, fail)


# ------------------------------------------------------------------------------------------------ the estimator calls, (f)
def particle_case():
    m, task, mocap, x0, ctrls, ys, ABCD = particle_imu_run()
    be = HipBackend(m, task, max_samples=16, max_horizon=2)

    def step(S, U, T):
        o = be.step_batch(S, U, T, mocap=mocap)
        return o["next_states"], o["residual"], o["failure"]
    return m, task, mocap, x0, ctrls, ys, ABCD, be, step


def test_linearize_step_and_unscented_moments_on_the_imu_table():
    """a model without a quaternion: the calls are the mirror's bits over the device's own step_batch, and the stepped rows
    the emulation's within the bar of (a)"""
    m, task, mocap, x0, ctrls, ys, ABCD, be, step = particle_case()
    x = x0 + np.array([0.01, -0.02, 0.05, 0.03]); u = ctrls[0]; t = 0.05
    out = be.linearize_step(x, u, t, mocap=mocap, eps=1e-6, centered=True)
    mir = em.Mirror(m, task, 0, 5)
    A, B, Cm, D, fail, _ = mir.fd.fd(step, x[None], u[None], np.array([t]), 1e-6, True)
    nxt, res, fl = step(x[None], u[None], np.array([t]))
    assert out["failure"] == 0 and np.array_equal(out["A"], A[0]) and np.array_equal(out["C"], Cm[0])
    assert np.array_equal(out["next_state"], nxt[0]) and np.array_equal(out["residual"], res[0])
    enxt, eres, efl = el.step_batch(m, task, x[None], u[None], np.array([t]), mocap)
    bar = max(lc.KIN_BAR["particle_imu"], lc.QACC_BAR["particle_imu"])      # the accelerometer rows are qacc's, permuted: qacc's bar
    print("imu rows, device against emulation", ck.dev(res, eres), "bar", bar, "next state", ck.dev(nxt, enxt))
    assert ck.dev(res, eres) <= bar
    _, _, Cc, _, _ = ABCD
    assert np.abs(out["C"] - Cc).max() <= 1e-8                    # the accelerometer rows of C: -damping / mass, through Rᵀ (central differences, eps 1e-6)
    L = em.chol(ec.covariance("particle")); w = em.weights(4); q = np.full(4, 1e-4); r = np.full(5, 1e-4) * (1 + 0.2 * np.arange(5))
    ref = mir.moments(step, x, L, w, u, t, q, r)
    got = be.unscented_moments(x, L, w["sigma_step"], (w["mean0"], w["cov0"], w["sigma"]), u, t, q, r, sensor_first_row=0, num_sensor=5, mocap=mocap)
    assert got["failure"] == 0 and all(np.array_equal(got[k], ref[k]) for k in ("state_mean", "sensor_mean", "cov_ss", "cov_sy", "cov_yy", "sigma_next"))
    assert np.abs(got["cov_sy"][:, 2:]).max() > 1e-6              # the accelerometer is correlated with the state
    be.close()


def test_particle_with_accelerometer_closed_form():
    m, task, mocap, x0, ctrls, ys, ABCD, be, step = particle_case()
    filters = dict(ekf=E.Kalman(be, 0, 5, epsilon=1e-6, flg_centered=True), ukf=E.Unscented(be, 0, 5))
    for f in filters.values():
        f.Reset(x0)
        if mocap is not None:
            f.SetShared(mocap=mocap)
    worst, x = closed_form_deviation(filters, x0, ctrls, ys, ABCD)
    print("particle with accelerometer, closed form", worst, "bar", lc.ESTIMATOR_BAR)
    assert np.abs(x - x0).max() > 1e-2 and max(worst.values()) <= lc.ESTIMATOR_BAR
    for f in filters.values():
        f.close()
    be.close()


# ------------------------------------------------------------------------------------------------ (e), unchanged behaviour
def test_plan_writes_late_rows_as_zero():
    c = lc.touch("twoball_elliptic"); m = c["model"]
    with_late, without, late_rows = _mixed_tables(m)
    outs = []
    for task in (with_late, without):
        be = HipBackend(m, task, max_samples=2, max_horizon=3)
        outs.append(be.plan(state=c["X"][1], mocap=np.zeros(0), time=0.0, knot_times=np.array([0.0]), knot_values=np.zeros((1, m["nu"])), interpolation=0,
                            num_trajectory=2, horizon=3, sigma=(0.0, 0.0)))
        if task is with_late:
            st = be.step_batch(c["X"], c["U"], c["T"])
        be.close()
    res = outs[0]["residual"]                                     # the winner's rows [H, nr]
    early = np.setdiff1d(np.arange(res.shape[1]), late_rows)
    assert res.shape[0] == 3 and np.array_equal(res[:, late_rows], np.zeros((3, len(late_rows)))) and np.abs(res[:, early]).max() > 0.05
    assert np.array_equal(res[:, early], outs[1]["residual"][:, early]) and np.array_equal(outs[0]["states"], outs[1]["states"])
    assert np.array_equal(outs[0]["returns"], outs[1]["returns"]) and not outs[0]["failure"].any()
    assert np.all(st["residual"][:, late_rows[0]] > 0)            # the same engine's step fills them


@pytest.mark.parametrize("name", ["particle", "cartpole", "filter_arm", "quadruped"])
def test_tables_without_late_blocks_step_as_before(name):
    """no late block: no table, no phase.  The step is bit for bit the first step of mjpc_hip_plan(N = 1, H = 2, P = 1), whose kernels
    this feature does not touch; on the particle and the cartpole (where the device's contracted arithmetic rounds as the emulation's
    separate operations do) it is the emulation's step bit for bit as well"""
    c = ec.case(name); m = c["model"]
    assert el.late_blocks(m, c["task"]) == 0
    be = HipBackend(m, c["task"], max_samples=16, max_horizon=2)
    x, u, t = c["state"], c["ctrl"], c["time"]
    o = be.step_batch(x[None], u[None], np.array([t]), mocap=c["mocap"])
    p = be.plan(state=x, mocap=c["mocap"], time=t, knot_times=np.array([0.0]), knot_values=u[None], interpolation=0, num_trajectory=1, horizon=2,
                sigma=(0.0, 0.0), candidate_knots=u.reshape(1, 1, -1))
    be.close()
    assert not o["failure"].any() and np.array_equal(o["next_states"][0], p["states"][1]) and np.array_equal(o["residual"][0], p["residual"][0])
    if name in ("particle", "cartpole"):
        enxt, eres, efl = el.step_batch(m, c["task"], x[None], u[None], np.array([t]), c["mocap"])
        assert np.array_equal(o["next_states"], enxt) and np.array_equal(o["residual"], eres)
