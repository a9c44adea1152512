"""The estimator tests' models (TEST INFRASTRUCTURE ONLY), shared by the CPU tier and the GPU tier: the smallest shapes where each part of
the unscented moments and of the two filters can go wrong.

    particle    copy-state residual, nd = 4; the measurement is residual rows 0-1 of 4 (a row range inside a larger residual)
    cartpole    a table of qpos
    filter_arm  na > 0 (the act block of the state); the table carries cost-like rows (ctrl) first, the sensors (qpos, act) behind them
    sphere      a free sphere over a plane, nd = 12, one quaternion (not the identity), no contact at the start: framepos + framequat
    quadruped   the A1 standing: trunk position + the 12 joint positions, 15 sensors, nd = 36: 73 rows, contacts, identity quaternion
"""
import functools

import numpy as np

import transition_cases as tc
import transition_mirror as tm
from mujoco_mpc_amd.modelgen.builder import FREE, PLANE, SPHERE, ModelBuilder
from mujoco_mpc_amd.modelgen.residual_table import ResidualTable

MODELS = ["particle", "cartpole", "filter_arm", "sphere", "quadruped"]
PLAIN = ["particle", "cartpole", "filter_arm"]          # no quaternion: bit-equal to the mirror


# Largest deviation of the EMULATION from the mirror relative to max(1, |entry|), measured on the CPU (tests/test_estimators.py prints each
# figure and says what it covers), and the bars of ten times that, shared by the CPU tier and the GPU tier
SIGMA_QUAT_MEASURED = {"sphere": 2.3e-16, "quadruped": 1.2e-16}         # the kernel's spelling against MuJoCo's (the table itself is bit-equal)
MOMENTS_MEASURED = {"sphere": 2.3e-16, "quadruped": 1.2e-16}
UPDATE_MEASURED = {"sphere": 2.3e-16, "quadruped": 1.2e-16}
KALMAN_COVARIANCE_MEASURED = {"sphere": 2.2e-12, "quadruped": 3.0e-12}     # not emulation against mirror: see the test of that name
QUAT_MEAN_MEASURED = 8.9e-16
CLOSED_FORM_MEASURED = 2.9e-14
SIGMA_QUAT_BAR = {k: 10 * v for k, v in SIGMA_QUAT_MEASURED.items()}
MOMENTS_BAR = {k: 10 * v for k, v in MOMENTS_MEASURED.items()}
UPDATE_BAR = {k: 10 * v for k, v in UPDATE_MEASURED.items()}
KALMAN_COVARIANCE_BAR = {k: 10 * v for k, v in KALMAN_COVARIANCE_MEASURED.items()}
QUAT_MEAN_BAR = 10 * QUAT_MEAN_MEASURED
CLOSED_FORM_BAR = 10 * CLOSED_FORM_MEASURED
assert CLOSED_FORM_BAR <= 1e-10


def _sphere():
    b = ModelBuilder()
    b.geom(0, "floor", PLANE, size=(1, 1, 0.1))
    body = b.body("ball", 0, pos=(0, 0, 1))
    b.joint(body, "f", FREE)
    b.geom(body, "g", SPHERE, size=(0.1,))
    m = b.compile()
    t = ResidualTable(m)
    t.sum(t.pos("xbody", "ball")); t.sum(t.quat("xbody", "ball"))
    q = np.array([0.8, 0.2, -0.4, 0.4]); q /= np.linalg.norm(q)
    state = np.concatenate([[0.1, -0.2, 1.0], q, [0.3, -0.1, 0.2], [0.5, -1.0, 0.7]])
    return m, t.measurement(), state, None


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(model, task, state, mocap, first, ns, ctrl, time)"""
    if name == "sphere":
        m, task, state, mocap = _sphere()
    else:
        m, task0, d = tc.model("particle_copystate" if name == "particle" else name)
        state = np.asarray(d["state"], float)
        mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
        t = ResidualTable(m)
        if name == "particle":
            task = task0
        elif name == "cartpole":
            t.sum(t.qpos()); task = t.measurement()
        elif name == "filter_arm":
            t.sum(t.ctrl()); t.sum(t.qpos()); t.sum(t.act()); task = t.measurement()
        else:
            t.sum(t.pos("xbody", "trunk")); t.sum(t.qpos()[7:19]); task = t.measurement()
    dd = tm.dims(m, task)
    first = dd["nu"] if name == "filter_arm" else 0
    ns = 2 if name == "particle" else dd["nr"] - first
    rng = np.random.default_rng(7)
    ctrl = rng.uniform(-0.3, 0.3, dd["nu"])
    if name in ("cartpole", "filter_arm"):                # off the rest pose: every coordinate moves
        state = state.copy()
        state[dd["nq"]:] += 0.05 * rng.standard_normal(dd["ds"] - dd["nq"])
    return dict(model=m, task=task, state=state, mocap=mocap, first=first, ns=ns, ctrl=ctrl, time=0.05, dims=dd)


def covariance(name, scale=1e-4, seed=3):
    """a full SPD covariance of the model's size (so that every column of its factor has entries below the diagonal)"""
    nd = case(name)["dims"]["nd"]
    G = np.random.default_rng(seed).standard_normal((nd, nd))
    return scale * (np.eye(nd) + 0.3 * (G @ G.T) / nd)


def quaternion_sets(n=1000, rows=25, seed=11):
    """n sets of `rows` unit quaternions spread by rotation vectors of up to 0.5 rad around a random centre; the last row is the centre
    turned like the others (it plays the nominal row)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, rows, 4))
    for s in range(n):
        c = rng.standard_normal(4); c /= np.linalg.norm(c)
        for j in range(rows):
            v = rng.standard_normal(3); v *= rng.uniform(0, 0.5) / np.linalg.norm(v)
            a = np.linalg.norm(v)
            r = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * v / a])
            out[s, j] = [c[0] * r[0] - c[1] * r[1] - c[2] * r[2] - c[3] * r[3], c[0] * r[1] + c[1] * r[0] + c[2] * r[3] - c[3] * r[2],
                         c[0] * r[2] - c[1] * r[3] + c[2] * r[0] + c[3] * r[1], c[0] * r[3] + c[1] * r[2] - c[2] * r[1] + c[3] * r[0]]
    return out


def particle_closed_form(m):
    """A, B of test_transition.py::test_particle_closed_form, C = [I 0]"""
    h = m["timestep"]; d = float(np.asarray(m["dof_damping"])[0])
    mass = float(np.asarray(m["body_mass"]).ravel()[-1]) + float(np.asarray(m["dof_armature"])[0]); gear = float(np.asarray(m["actuator_gear"]).ravel()[0])
    a = 1 - h * d / (mass + h * d)
    I2, Z2 = np.eye(2), np.zeros((2, 2))
    A = np.block([[I2, h * a * I2], [Z2, a * I2]]); B = gear * np.vstack([h * h / (mass + h * d) * I2, h / (mass + h * d) * I2])
    return A, B, np.hstack([I2, Z2])


def particle_run(updates=20, seed=5, scale=1e-4):
    """truth states by the closed form from tc.batch("particle_copystate")'s row 1, seeded controls in +-0.3, seeded measurement noise"""
    m, task, mocap, X, U, T = tc.batch("particle_copystate", n=2, spread=0.5)
    A, B, Cm = particle_closed_form(m)
    rng = np.random.default_rng(seed)
    x = X[1].copy()
    ctrls = rng.uniform(-0.3, 0.3, (updates, 2)); ys = np.zeros((updates, 2))
    for k in range(updates):
        ys[k] = Cm @ x + np.sqrt(scale) * rng.standard_normal(2)
        x = A @ x + B @ ctrls[k]
    return m, task, mocap, X[0].copy(), ctrls, ys, (A, B, Cm)
