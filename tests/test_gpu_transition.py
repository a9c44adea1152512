"""GPU tier of the batched one-step evaluation (mjpc_hip_step_batch) and the finite-difference transition derivatives
(mjpc_hip_transition_fd, mjpc_hip::ModelDerivatives): steps bit-identical to plain plans in every kernel flavour, chunking, the
derivatives against the numpy mirror over step_batch (bars of tests/test_transition.py), the particle's closed form, nudges,
terminal knot, a NaN state, misuse, and the C++ class through its C view."""
import numpy as np
import pytest

import transition_cases as tc
import transition_mirror as tm
from mujoco_mpc_amd.derivatives import ModelDerivatives
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

QUAT_BAR = 1e-8          # ball / free-rotation rows: a few dozen ulp of atan2 / sin divided by eps = 1e-6, relative to max(1, |entry|)


def _backend(m, task, max_samples=256, max_horizon=2):
    return HipBackend(m, task, max_samples=max_samples, max_horizon=max_horizon)


def _step_fn(be, mocap):
    def step(S, U, T):
        o = be.step_batch(S, U, T, mocap=mocap)
        return o["next_states"], o["residual"], o["failure"]
    return step


def _check_against_mirror(out, ref, qrows):
    A, B, C, D, fail, _ = ref
    plain = ~qrows
    assert np.array_equal(out["A"][:, plain], A[:, plain], equal_nan=True) and np.array_equal(out["B"][:, plain], B[:, plain], equal_nan=True)
    assert np.array_equal(out["C"], C, equal_nan=True) and np.array_equal(out["D"], D, equal_nan=True)
    for got, want in ((out["A"][:, qrows], A[:, qrows]), (out["B"][:, qrows], B[:, qrows])):
        if got.size:
            dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            print("quaternion rows: largest deviation", np.nanmax(dev))
            assert np.nanmax(dev) <= QUAT_BAR and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(out["failure"], fail)


@pytest.mark.parametrize("name", ["particle", "quadruped", "filter_arm", "humanoid_spill"])
def test_step_batch_is_bit_identical_to_plain_plans(name):
    m, task, mocap, X, U, T = tc.batch(name, n=5)
    be = _backend(m, task, max_samples=8)
    assert (be.spill_bytes() > 0) == (name == "humanoid_spill")
    out = be.step_batch(X, U, T, mocap=mocap)
    for i in range(5):
        p = be.plan(state=X[i], mocap=mocap, time=T[i], knot_times=np.array([0.0]), knot_values=U[i:i + 1], interpolation=0, num_trajectory=1,
                    horizon=2, sigma=(0.0, 0.0), candidate_knots=U[i].reshape(1, 1, -1))
        assert np.array_equal(out["next_states"][i], p["states"][1]), i
        assert np.array_equal(out["residual"][i], p["residual"][0]), i
        assert out["failure"][i] == p["failure"][0] == 0, i
    # distinct rows came out distinct, and a second call repeats the first bit for bit
    assert len({r.tobytes() for r in out["next_states"]}) == 5
    again = be.step_batch(X, U, T, mocap=mocap)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    be.close()


def test_chunked_transition_fd_equals_one_launch():
    """A1, T = 2, centred: 2 * (1 + 2 * 48) = 194 evaluations; 25 launches of at most 8 workgroups against one launch"""
    m, task, mocap, X, U, T = tc.batch("quadruped", n=2)
    outs = []
    for cap in (8, 256):
        be = _backend(m, task, max_samples=cap)
        outs.append(be.transition_fd(X, U, T, mocap=mocap, eps=1e-6, centered=True))
        be.close()
    for k in "ABCD":
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(outs[0]["failure"], outs[1]["failure"]) and not outs[0]["failure"].any()
    assert np.abs(outs[0]["A"]).max() > 0.5


@pytest.mark.parametrize("name", ["quadruped", "filter_arm"])
@pytest.mark.parametrize("centered", [False, True])
def test_transition_fd_matches_mirror_over_step_batch(name, centered):
    m, task, mocap, X, U, T = tc.batch(name, n=2)
    be = _backend(m, task)
    mir = tm.Mirror(m, task)
    out = be.transition_fd(X, U, T, mocap=mocap, eps=1e-6, centered=centered)
    ref = mir.fd(_step_fn(be, mocap), X, U, T, 1e-6, centered)
    _check_against_mirror(out, ref, ref[5])
    be.close()


@pytest.mark.parametrize("centered", [False, True])
def test_particle_closed_form(centered):
    """Two slide joints under Euler with implicit damping: a = 1 - h d / (m + h d), A = [[I, h a I], [0, a I]], B = [[h^2 / (m + h d) I],
    [h / (m + h d) I]]; copy-state residual: C = I, D = 0.  Linear, so FD is exact up to ulp / eps: 1e-8 absolute at eps = 1e-6."""
    m, task, mocap, X, U, T = tc.batch("particle_copystate", n=2, spread=0.5)
    h = m["timestep"]; d = float(np.asarray(m["dof_damping"])[0]); mass = float(np.asarray(m["body_mass"]).ravel()[-1]) + float(np.asarray(m["dof_armature"])[0])
    gear = float(np.asarray(m["actuator_gear"]).ravel()[0])
    a = 1 - h * d / (mass + h * d)
    I2, Z2 = np.eye(2), np.zeros((2, 2))
    A = np.block([[I2, h * a * I2], [Z2, a * I2]]); B = gear * np.vstack([h * h / (mass + h * d) * I2, h / (mass + h * d) * I2])
    be = _backend(m, task)
    out = be.transition_fd(X, U, T, mocap=mocap, eps=1e-6, centered=centered)
    be.close()
    for t in range(2):
        for got, want in ((out["A"][t], A), (out["B"][t], B), (out["C"][t], np.eye(4)), (out["D"][t], np.zeros((4, 2)))):
            assert np.abs(got - want).max() <= 1e-8
    assert not out["failure"].any()


@pytest.mark.parametrize("centered", [False, True])
def test_control_nudges_and_terminal_knot(centered):
    """filter_arm with its ctrlranges rewritten: one actuator at hi, one at lo, one inside, one with hi - lo < eps (a zero column)"""
    m, task, mocap, X, U, T = tc.batch("filter_arm", n=3)
    m, U, eps = tc.nudge_case(m, U)
    be = _backend(m, task)
    mir = tm.Mirror(m, task)
    fl = mir.flags(U[0], eps, centered)
    assert fl[:4] == [(False, True), (True, False), (True, centered), (False, False)]
    out = be.transition_fd(X, U, T, mocap=mocap, eps=eps, centered=centered, last_is_terminal=True, fill=np.nan)
    ref = mir.fd(_step_fn(be, mocap), X, U, T, eps, centered, last_is_terminal=True)
    _check_against_mirror(out, ref, ref[5])
    nd = tm.dims(m, task)["nd"]
    assert np.all(out["B"][:2, :, 3] == 0) and np.all(out["D"][:2, :, 3] == 0) and np.abs(out["B"][:2, :, :3]).max() > 0
    assert np.isnan(out["A"][2]).all() and np.isnan(out["B"][2]).all() and np.isnan(out["D"][2]).all()      # terminal: untouched
    assert np.isfinite(out["C"]).all() and np.isfinite(out["A"][:2]).all() and out["C"].shape[2] == nd
    be.close()


def test_batches_larger_than_one_pass_of_the_device_tables():
    """the device tables hold at most 32 768 rows; a larger n / T runs pass after pass.  Particle: 33 000 steps, and 2 600 knots centred
    (13 evaluations each: 33 800 rows), against the same rows / knots in small calls"""
    m, task, mocap, X, U, T = tc.batch("particle", n=64)
    be = _backend(m, task, max_samples=4096)
    n = 33000
    idx = np.arange(n) % 64
    big = be.step_batch(X[idx], U[idx], T[idx], mocap=mocap)
    small = be.step_batch(X, U, T, mocap=mocap)
    assert np.array_equal(big["next_states"], small["next_states"][idx]) and np.array_equal(big["residual"], small["residual"][idx]) and not big["failure"].any()
    nk = 2600
    idx = np.arange(nk) % 64
    fd_big = be.transition_fd(X[idx], U[idx], T[idx], mocap=mocap, eps=1e-6, centered=True, last_is_terminal=True, fill=np.nan)
    fd_small = be.transition_fd(X, U, T, mocap=mocap, eps=1e-6, centered=True)
    for k in "ABD":
        assert np.array_equal(fd_big[k][:-1], fd_small[k][idx[:-1]]) and np.isnan(fd_big[k][-1]).all(), k
    assert np.array_equal(fd_big["C"], fd_small["C"][idx]) and not fd_big["failure"].any()
    be.close()


def test_nan_state_is_a_flagged_row_not_a_fault():
    m, task, mocap, X, U, T = tc.batch("quadruped", n=5)
    be = _backend(m, task, max_samples=8)
    good = be.step_batch(X, U, T, mocap=mocap)
    Xb = X.copy(); Xb[2, 1] = np.nan
    bad = be.step_batch(Xb, U, T, mocap=mocap)
    assert bad["failure"][2] & 1 and not bad["failure"][[0, 1, 3, 4]].any()            # MJPC_WARN_BADQPOS, that row only
    for i in (0, 1, 3, 4):
        assert np.array_equal(bad["next_states"][i], good["next_states"][i]) and np.array_equal(bad["residual"][i], good["residual"][i])
    assert np.isnan(bad["residual"][2]).all()
    # the same through the derivatives: the knot with the NaN state is flagged, the other knot's blocks are those of a clean call
    fd_good = be.transition_fd(X[:2], U[:2], T[:2], mocap=mocap, eps=1e-6)
    fd_bad = be.transition_fd(np.vstack([Xb[2], X[1]]), U[[2, 1]], T[[2, 1]], mocap=mocap, eps=1e-6)
    assert fd_bad["failure"][0] & 1 and fd_bad["failure"][1] == 0
    assert all(np.array_equal(fd_bad[k][1], fd_good[k][1]) for k in "ABCD")
    be.close()


def test_calls_during_a_pending_plan_are_refused_and_the_plan_stays_fetchable():
    m, task, mocap, X, U, T = tc.batch("particle", n=3)
    be = _backend(m, task, max_samples=4, max_horizon=4)
    kt = np.array([0.0, 0.2]); kv = np.zeros((2, m["nu"]))
    kw = dict(state=X[0], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=1, num_trajectory=4, horizon=4, sigma=(0.1, 0.0), seed=3)
    ref = be.plan(**kw)
    inp = be.make_input(**kw)
    be.plan_async(inp)
    with pytest.raises(RuntimeError, match="in flight"):
        be.step_batch(X, U, T, mocap=mocap)
    with pytest.raises(RuntimeError, match="in flight"):
        be.transition_fd(X, U, T, mocap=mocap)
    got = be.plan_fetch(inp)
    assert np.array_equal(got["returns"], ref["returns"]) and np.array_equal(got["states"], ref["states"]) and got["winner"] == ref["winner"]
    for bad, msg in ((dict(eps=0.0), "eps"), (dict(eps=-1e-6), "eps")):
        with pytest.raises(RuntimeError, match=msg):
            be.transition_fd(X, U, T, mocap=mocap, **bad)
    with pytest.raises(RuntimeError, match="n < 1"):
        be.step_batch(X[:0], U[:0], T[:0], mocap=mocap)
    be.close()
    one = _backend(m, task, max_samples=4, max_horizon=1)
    with pytest.raises(RuntimeError, match="max_horizon"):
        one.step_batch(X, U, T, mocap=mocap)
    one.close()


def test_model_derivatives_class_on_the_particle():
    """T = 5, skip = 1: evaluated {0, 2, 3, 4}, index 1 interpolated half-way between 0 and 2; index 4 terminal (C only)"""
    m, task, mocap, X, U, T = tc.batch("particle", n=5)
    be = _backend(m, task)
    md = ModelDerivatives(m, task, T=5)
    out = md.compute(be, X, U, T, tol=1e-6, mode=1, skip=1, mocap=mocap)
    ev, plan = tm.interpolate_plan(5, 1)
    assert list(out["evaluate"]) == ev == [0, 2, 3, 4] and list(out["interpolate"]) == [1] and plan == [(1, 0, 2, 0.5)]
    direct = be.transition_fd(X[ev], U[ev], T[ev], mocap=mocap, eps=1e-6, centered=True, last_is_terminal=True, fill=0.0)
    for k in "ABCD":
        for j, t in enumerate(ev):
            assert np.array_equal(out[k][t], direct[k][j]), (k, t)
        assert np.array_equal(out[k][1], tm.interpolate(out[k][0], out[k][2], 0.5)), k
    assert not out["A"][4].any() and not out["B"][4].any() and not out["D"][4].any() and out["C"][4].any()
    assert not out["failure"].any()
    with pytest.raises(RuntimeError, match="T < 2"):          # cplanner.PlannerError, where the reference aborts through mju_error
        md.compute(be, X[:1], U[:1], T[:1])
    md.close(); be.close()
