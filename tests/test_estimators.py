"""CPU tier of the state estimators: the unscented-moments kernels (csrc/estimator.h) in the 1-lane emulation against the numpy mirror
(tests/estimator_mirror.py), the quaternion mean against numpy.linalg.eigh, the host filter algebra (csrc/planner.cc) against the mirror
and numpy, and both filters on the particle against the textbook Kalman filter.

Bars.  The sigma-point table is BIT-EQUAL to the mirror on every model, quaternions included (ukf_quatintegrate is spelled so that its
bits do not depend on who computes it), and so are the stepped rows.  Models without a quaternion (particle, cartpole, filter_arm) are
bit-equal in every quantity.  On the sphere and the A1 the quaternion mean (QUEST iteration against eigh) and the quaternion differences
differ by rounding; the largest deviation of the emulation from the mirror relative to max(1, |entry|), measured on the CPU, and the
bar of ten times that:
    sigma table, quaternion coordinates against MuJoCo's spelling in numpy (scale 0.05: turns of up to 0.8 rad)   sphere 2.3e-16   A1 1.2e-16
    means, difference table, covariance blocks (covariance scale 1e-4)                          sphere 2.3e-16   A1 1.2e-16
    one unscented update from those moments: state and covariance                               sphere 2.3e-16   A1 1.2e-16
    covariance of one Kalman update when A's quaternion rows move by the device's 1e-8 bar      sphere 2.2e-12   A1 3.0e-12
    quaternion mean of 1000 sets of 25 against eigh                                             8.9e-16
    particle, 20 updates against the textbook Kalman filter (state and covariance)              EKF 2.9e-14  UKF 2.1e-17 (centred, eps = 1e-6)
None of these is derived from device output."""
import numpy as np
import pytest

import emu_estimator_lib as ee
import emu_transition_lib as et
import estimator_cases as ec
import estimator_mirror as em
from mujoco_mpc_amd import estimators as E
from mujoco_mpc_amd.modelgen.residual_table import ResidualTable

from estimator_cases import CLOSED_FORM_BAR, KALMAN_COVARIANCE_BAR, MOMENTS_BAR, QUAT_MEAN_BAR, SIGMA_QUAT_BAR, UPDATE_BAR      # measured here, shared with the GPU tier

# host algebra against numpy's LAPACK: two backward-stable solutions of systems of order <= 51 whose condition number the test keeps
# below 1e3 (asserted there) differ by at most about order * condition * 2^-52 = 51 * 1e3 * 2.2e-16
NUMPY_BAR = 1.2e-11
MOMENT_KEYS = ("state_mean", "sensor_mean", "diff", "cov_ss", "cov_sy", "cov_yy", "sigma_next")


def dev(got, want):
    return float(np.nanmax(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if np.size(got) else 0.0


def emu_step(c):
    return lambda S, U, T: et.step_batch(c["model"], c["task"], S, U, T, c["mocap"])


def emu_moments(c):
    def f(mir, x, L, w, u, time, q, r):
        return ee.unscented_moments(c["model"], c["task"], x, L, w["sigma_step"], [w["mean0"], w["cov0"], w["sigma"]], u, time, q, r, mir.first, mir.ns,
                                    c["mocap"])
    return f


def moments_inputs(name):
    c = ec.case(name); nd = c["dims"]["nd"]
    return c, em.chol(ec.covariance(name)), em.weights(nd), np.full(nd, 1e-4) * (1 + 0.1 * np.arange(nd)), np.full(c["ns"], 1e-4) * (1 + 0.2 * np.arange(c["ns"]))


@pytest.mark.parametrize("name", ec.MODELS)
def test_sigma_table_matches_mirror(name):
    c = ec.case(name); nd = c["dims"]["nd"]
    L = em.chol(ec.covariance(name, scale=0.05)); w = em.weights(nd)
    L = L + np.triu(np.full((nd, nd), np.nan), 1)                    # entries above the diagonal read as 0: never loaded
    mir = em.Mirror(c["model"], c["task"], c["first"], c["ns"])
    S, U, T = mir.sigma_table(c["state"], np.tril(np.nan_to_num(L)), w["sigma_step"], c["ctrl"], c["time"])
    eS, eU, eT = ee.sigma_table(c["model"], c["task"], c["state"], L, c["ctrl"], w["sigma_step"], c["time"])
    q = mir.quat_state
    assert np.array_equal(eS, S) and np.array_equal(eU, U) and np.array_equal(eT, T)          # every coordinate, quaternions included
    assert np.array_equal(eS[-1], c["state"]) and not np.array_equal(eS[0], eS[nd]) and np.isfinite(eS).all()
    assert q.any() == (name in SIGMA_QUAT_BAR)
    if q.any():
        # the kernel's spelling of the quaternion integration against MuJoCo's in numpy's functions
        M, _, _ = mir.sigma_table(c["state"], np.tril(np.nan_to_num(L)), w["sigma_step"], c["ctrl"], c["time"], quat=em.quat_integrate_mujoco)
        d = dev(eS[:, q], M[:, q])
        print(name, "sigma table, quaternion coordinates against MuJoCo's spelling", d, "bar", SIGMA_QUAT_BAR[name])
        assert d <= SIGMA_QUAT_BAR[name] and np.array_equal(eS[:, ~q], M[:, ~q])
        assert np.abs(np.linalg.norm(eS[:, mir.quats[0]:mir.quats[0] + 4], axis=1) - 1).max() < 1e-15


def test_sincos_of_the_sigma_table():
    """ukf_sincos restated (estimator_mirror.sincos_rn) against the library over the half-angles a sigma point can have and beyond"""
    x = np.concatenate([np.linspace(-3.2, 3.2, 20001), np.random.default_rng(0).uniform(-60, 60, 20000), [0.0, 1e-300, -1e-9, 63.999]])
    got = np.array([em.sincos_rn(float(v)) for v in x])
    ulp = np.spacing(1.0)
    assert np.abs(got[:, 0] - np.sin(x)).max() <= 2 * ulp and np.abs(got[:, 1] - np.cos(x)).max() <= 2 * ulp


@pytest.mark.parametrize("name", ec.MODELS)
def test_moments_match_mirror_over_emulated_steps(name):
    c, L, w, q, r = moments_inputs(name)
    mir = em.Mirror(c["model"], c["task"], c["first"], c["ns"])
    o = mir.moments(emu_step(c), c["state"], L, w, c["ctrl"], c["time"], q, r)
    e = emu_moments(c)(mir, c["state"], L, w, c["ctrl"], c["time"], q, r)
    assert e["failure"] == 0 and o["failure"] == 0
    assert all(np.isfinite(e[k]).all() for k in MOMENT_KEYS)         # every entry of every block was written (the outputs start as NaN)
    for k in MOMENT_KEYS if name in ec.PLAIN else ("sigma_next", "sensor_mean", "cov_yy"):
        assert np.array_equal(e[k], o[k]), k
    if name not in ec.PLAIN:
        worst = max(dev(e[k], o[k]) for k in MOMENT_KEYS)
        print(name, "moments", {k: dev(e[k], o[k]) for k in MOMENT_KEYS}, "bar", MOMENTS_BAR[name])
        assert worst <= MOMENTS_BAR[name]
        qa = mir.quats[0]
        assert abs(np.linalg.norm(e["state_mean"][qa:qa + 4]) - 1) < 1e-14 and e["state_mean"][qa:qa + 4] @ e["sigma_next"][-1, qa:qa + 4] > 0
    # the noise sits on the diagonals and nowhere else: without it the blocks are the plain weighted sums
    z = emu_moments(c)(mir, c["state"], L, w, c["ctrl"], c["time"], np.zeros_like(q), np.zeros_like(r))
    assert np.allclose(e["cov_ss"] - z["cov_ss"], np.diag(q), rtol=0, atol=1e-15) and np.allclose(e["cov_yy"] - z["cov_yy"], np.diag(r), rtol=0, atol=1e-15)
    assert np.array_equal(e["cov_sy"], z["cov_sy"]) and np.array_equal(e["cov_ss"], e["cov_ss"].T) and np.array_equal(e["cov_yy"], e["cov_yy"].T)


@pytest.mark.parametrize("name", ["sphere", "quadruped"])
def test_one_unscented_update_from_emulated_moments(name):
    """the filter's algebra does not blow the moments' deviation up: one update of the mirror from the emulated moments against one from
    its own (the bar of the GPU tier's class test on these models)"""
    c = ec.case(name)
    nxt, res, fail = emu_step(c)(c["state"][None], c["ctrl"][None], np.array([c["time"]]))
    # a measurement: the sensors at the state itself plus seeded noise of the filter's scale (variance 1e-4)
    y = res[0, c["first"]:c["first"] + c["ns"]] + 1e-2 * np.random.default_rng(2).standard_normal(c["ns"])
    out = []
    for moments in (None, emu_moments(c)):
        f = em.Unscented(c["model"], c["task"], emu_step(c), c["first"], c["ns"])
        f.Reset(c["state"], c["time"])
        f.covariance = ec.covariance(name)             # full: the sigma points turn about every axis at once
        assert f.Update(c["ctrl"], y, moments=moments) == em.OK
        out.append((f.state.copy(), f.covariance.copy()))
    d = max(dev(out[1][0], out[0][0]), dev(out[1][1], out[0][1]))
    print(name, "one update", d, "bar", UPDATE_BAR[name])
    assert d <= UPDATE_BAR[name] and np.abs(out[0][0] - c["state"]).max() > 1e-4


@pytest.mark.parametrize("name", ["sphere", "quadruped"])
def test_one_kalman_update_under_the_quaternion_row_bar(name):
    """The extended filter on a model with a quaternion.  The emulated transition_fd equals the mirror's bit for bit at these states (both
    take atan2 from the same library), so the emulation says nothing about a device whose quaternion ROWS of A may differ by QUAT_BAR =
    1e-8 max(1, |entry|) (tests/test_gpu_transition.py); C has no such rows and is bit-equal there.  What such a change of A does to the
    covariance of one update is measured instead: every quaternion row moved by the full bar with seeded signs (not the worst case of
    signs, hence ten times it as well).  The state does not
    depend on A."""
    c = ec.case(name)
    step = emu_step(c)
    nxt, res, fail = step(c["state"][None], c["ctrl"][None], np.array([c["time"]]))
    y = res[0, c["first"]:c["first"] + c["ns"]] + 1e-2 * np.random.default_rng(2).standard_normal(c["ns"])
    mir = em.Mirror(c["model"], c["task"], c["first"], c["ns"])
    rows = mir.quat_cols
    assert rows.sum() == 3

    def emu_linearize(x, u, t, eps, centered, move=0.0):
        A, B, C, D, fl = et.transition_fd(c["model"], c["task"], x[None], u[None], np.array([t]), c["mocap"], eps, centered)
        n, r, f = step(x[None], u[None], np.array([t]))
        A = A[0].copy()
        sign = np.random.default_rng(4).choice([-1.0, 1.0], A[rows].shape)
        A[rows] += move * sign * np.maximum(1.0, np.abs(A[rows]))
        return A, C[0], n[0], r[0], int(fl[0])
    out = []
    for lin in (None, emu_linearize, lambda *a: emu_linearize(*a, move=1e-8)):
        f = em.Kalman(c["model"], c["task"], step, c["first"], c["ns"], eps=1e-6, centered=True)
        f.linearize = lin
        f.Reset(c["state"], c["time"])
        f.covariance = ec.covariance(name)
        assert f.Update(c["ctrl"], y) == em.OK
        out.append((f.state.copy(), f.covariance.copy()))
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])          # emulated derivatives: the mirror's bits
    assert np.array_equal(out[2][0], out[0][0]) and np.abs(out[0][0] - c["state"]).max() > 1e-4
    d = dev(out[2][1], out[0][1])
    print(name, "covariance of one kalman update under QUAT_BAR", d, "bar", KALMAN_COVARIANCE_BAR[name])
    assert 0 < d <= KALMAN_COVARIANCE_BAR[name]


def test_quaternion_mean_against_eigh():
    Q = ec.quaternion_sets(); w = em.weights(12)
    wc = np.full(25, w["sigma"]); wc[-1] = w["cov0"]
    worst = 0.0
    for s in range(Q.shape[0]):
        rows = np.zeros((25, 13)); rows[:, 3:7] = Q[s]
        got = ee.quat_mean(7, 6, 0, 3, rows, w["cov0"], w["sigma"])
        ref = em.quat_mean_eigh(Q[s], wc, Q[s, -1])
        assert got @ Q[s, -1] >= 0                                    # the sign rule
        worst = max(worst, float(np.abs(got - ref).max()))
    print("quaternion mean against eigh", worst, "bar", QUAT_MEAN_BAR)
    assert worst <= QUAT_MEAN_BAR
    # the degenerate set: identical quaternions come back (a generic one, the identity, a half turn about x: the last component of the
    # [w x y z] order vanishes in the latter two, where the reference's formula is 0 / 0)
    for q in (Q[0, 0], np.array([1.0, 0, 0, 0]), np.array([0.0, 1, 0, 0]), -Q[1, 3]):
        rows = np.zeros((25, 13)); rows[:, 3:7] = q
        assert np.abs(ee.quat_mean(7, 6, 0, 3, rows, w["cov0"], w["sigma"]) - q).max() <= QUAT_MEAN_BAR


@pytest.mark.parametrize("nd,ns", [(4, 2), (12, 3), (36, 15)])
def test_host_algebra(nd, ns):
    rng = np.random.default_rng(nd)
    G = rng.standard_normal((nd, nd)); P = G @ G.T / nd + 0.1 * np.eye(nd)
    Cm = rng.standard_normal((ns, nd)); R = rng.uniform(0.1, 1, ns); A = rng.standard_normal((nd, nd)); Q = rng.uniform(0.1, 1, nd); err = rng.standard_normal(ns)
    M = rng.standard_normal((nd + ns, nd + ns + 5)); V = M @ M.T / (nd + ns) + 0.1 * np.eye(nd + ns)
    S = Cm @ P @ Cm.T + np.diag(R)
    assert max(np.linalg.cond(P), np.linalg.cond(S), np.linalg.cond(V)) < 1e3
    # the gain and the correction
    rc, PCt, F, K = E.kalman_gain(P, Cm, R)
    mrc, mPCt, mF, mK = em.kalman_gain(P, Cm, R)
    assert rc == E.OK == mrc and np.array_equal(PCt, mPCt) and np.array_equal(F, mF) and np.array_equal(K, mK)
    Kn = P @ Cm.T @ np.linalg.inv(S)
    assert dev(K, Kn) <= NUMPY_BAR and np.array_equal(np.triu(F, 1), np.zeros_like(F))
    corr, P1 = E.kalman_correct(PCt, F, K, err, P)
    mcorr, mP1 = em.kalman_correct(mPCt, mF, mK, err, P)
    assert np.array_equal(corr, mcorr) and np.array_equal(P1, mP1) and np.array_equal(P1, P1.T)
    assert dev(corr, Kn @ err) <= NUMPY_BAR and dev(P1, P - Kn @ Cm @ P) <= NUMPY_BAR
    # the predict step
    Pp = E.covariance_predict(A, Q, P)
    assert np.array_equal(Pp, em.covariance_predict(A, Q, P)) and np.array_equal(Pp, Pp.T) and dev(Pp, A @ P @ A.T + np.diag(Q)) <= NUMPY_BAR * nd
    # the unscented correction
    rc, cu, Pu = E.unscented_correct(V[:nd, :nd], V[:nd, nd:], V[nd:, nd:], err)
    mrc, mcu, mPu = em.unscented_correct(V[:nd, :nd], V[:nd, nd:], V[nd:, nd:], err)
    Ku = V[:nd, nd:] @ np.linalg.inv(V[nd:, nd:])
    assert rc == E.OK == mrc and np.array_equal(cu, mcu) and np.array_equal(Pu, mPu) and np.array_equal(Pu, Pu.T)
    assert dev(cu, Ku @ err) <= NUMPY_BAR and dev(Pu, V[:nd, :nd] - Ku @ V[nd:, nd:] @ Ku.T) <= NUMPY_BAR
    st, Lf = E.covariance_factor(P)
    assert st == E.OK and np.array_equal(Lf, em.chol(P)) and dev(Lf, np.linalg.cholesky(P)) <= NUMPY_BAR
    # rank-deficient inputs: the status, and the outputs as they were handed in
    # (integers, so that the vanishing pivot is an exact zero and not a rounding residue of either sign)
    v = rng.integers(1, 5, nd).astype(float); Pr = np.outer(v, v)                       # rank one
    st, Lf = E.covariance_factor(Pr)
    assert st == E.COVARIANCE_RANK and np.isnan(Lf).all() and em.chol(Pr) is None
    u = rng.integers(1, 5, (ns, 1)).astype(float); Vr = u @ u.T                         # rank-one cov_yy
    rc, cu, Pu = E.unscented_correct(V[:nd, :nd], V[:nd, nd:], Vr, err, fill=7.0)
    assert rc == E.SENSOR_RANK and np.all(cu == 7.0) and np.all(Pu == 7.0) and em.unscented_correct(V[:nd, :nd], V[:nd, nd:], Vr, err)[0] == em.SENSOR_RANK
    Cr = np.zeros((ns, nd)); Cr[:, 0] = 3.0; Cr[:, 1] = 4.0                              # equal sensor rows, no sensor noise: C C' = 25 everywhere
    rc, PCt, F, K = E.kalman_gain(np.eye(nd), Cr, np.zeros(ns), fill=7.0)
    assert rc == E.SENSOR_RANK and np.all(PCt == 7.0) and np.all(F == 7.0) and np.all(K == 7.0)
    assert em.kalman_gain(np.eye(nd), Cr, np.zeros(ns))[0] == em.SENSOR_RANK


def test_particle_closed_form():
    """EKF and UKF of the mirror over emulated steps, 20 updates, against the textbook Kalman filter from the closed-form A, B, C = [I 0]"""
    m, task, mocap, x0, ctrls, ys, (A, B, Cm) = ec.particle_run()
    step = lambda S, U, T: et.step_batch(m, task, S, U, T, mocap)      # noqa: E731
    ekf = em.Kalman(m, task, step, 0, 2, eps=1e-6, centered=True); ukf = em.Unscented(m, task, step, 0, 2)
    ekf.Reset(x0); ukf.Reset(x0)
    x, P = x0.copy(), 1e-4 * np.eye(4)
    worst = {"ekf": 0.0, "ukf": 0.0}
    for k in range(len(ctrls)):
        x, P = em.textbook_kalman(A, B, Cm, 1e-4 * np.eye(4), 1e-4 * np.eye(2), x, P, ctrls[k], ys[k])
        assert ekf.Update(ctrls[k], ys[k]) == em.OK and ukf.Update(ctrls[k], ys[k]) == em.OK
        for key, f in (("ekf", ekf), ("ukf", ukf)):
            worst[key] = max(worst[key], float(np.abs(f.state - x).max()), float(np.abs(f.covariance - P).max()))
    print("particle closed form", worst, "bar", CLOSED_FORM_BAR)
    assert abs(ekf.time - 20 * m["timestep"]) < 1e-12 and np.abs(x - x0).max() > 1e-2          # the filters went somewhere
    assert worst["ekf"] <= CLOSED_FORM_BAR and worst["ukf"] <= CLOSED_FORM_BAR


def test_measurement_task_and_bindings():
    c = ec.case("cartpole")
    t = ResidualTable(c["model"]); t.sum(t.qpos()); t.sum(t.qvel()[1])
    task = t.measurement()
    assert task["num_residual"] == 3 and task["num_term"] == 1 and list(task["dim_norm_residual"]) == [3] and list(task["weight"]) == [0.0]
    L = E.lib()
    for s in E.ESTIMATOR_C_SYMBOLS:
        getattr(L, s)
    from mujoco_mpc_amd import capi
    from mujoco_mpc_amd.planner import HipBackend
    assert {"mjpc_hip_unscented_moments", "mjpc_hip_linearize_step"} <= set(capi.EXPORTED_SYMBOLS)
    assert callable(HipBackend.unscented_moments) and callable(HipBackend.linearize_step)
