"""Models, tables and states of the late-row tests (TEST INFRASTRUCTURE ONLY), shared by the CPU tier (tests/test_late_rows.py, the
emulation) and the GPU tier (tests/test_gpu_late_rows.py): the smallest shapes where each late kind can go wrong.

    chain3_euler / chain3_implicitfast   three hinges about different axes, a site offset from the last body and turned against it
    sphere                               a free sphere (nd = 12) spinning, contacts disabled: the quaternion path and ω × v
    filter_arm                           na > 0: the registry model with its tip site
    particle_imu                         the particle with a turned tip site: the rest reading, the bit-equal case, the estimator case
    twoball_elliptic / twoball_pyramidal one free body with two spheres resting on a plane: two contacts, one zone over one of them,
                                         one zone over both
    quadruped_elliptic / _pyramidal      the A1 of con_cases, states of its rollout, four foot zones; the front right foot starts in the air

The bars: ten times the largest deviation of the EMULATION from the references of tests/acc_ref.py relative to max(1, |entry|), measured
on the CPU (tests/test_late_rows.py prints each figure), shared by both tiers.  Never derived from device output.
"""
import functools

import numpy as np

import con_cases as cc
import transition_cases as tc
from mujoco_mpc_amd.modelgen import particle
from mujoco_mpc_amd.modelgen.builder import CAPSULE, FREE, HINGE, PLANE, SPHERE, ModelBuilder, axisangle2quat
from mujoco_mpc_amd.modelgen.residual_table import ResidualTable

KINEMATIC = ["chain3_euler", "chain3_implicitfast", "sphere", "filter_arm", "particle_imu"]
TOUCH = ["twoball_elliptic", "twoball_pyramidal", "quadruped_elliptic", "quadruped_pyramidal"]
FEET = [("FR", "FR"), ("FL", "FL"), ("RR", "HR"), ("RL", "HL")]            # (site, geom) of the A1's feet
FOOT_ZONE = ("sphere", (0.03,))                                           # the foot geoms are spheres of radius 0.02 around the sites

# measured on the CPU: emulation against acc_ref, relative to max(1, |entry|) (touch: max(1, |force|)); bars = ten times that
KIN_MEASURED = {"chain3_euler": 5.4e-15, "chain3_implicitfast": 5.4e-15, "sphere": 8.9e-15, "filter_arm": 2.4e-15, "particle_imu": 0.0}
QACC_MEASURED = {"chain3_euler": 1.7e-15, "chain3_implicitfast": 1.7e-15, "sphere": 3.4e-14, "filter_arm": 1.5e-14, "particle_imu": 1.2e-16}
TOUCH_MEASURED = {"twoball_elliptic": 1.5e-14, "twoball_pyramidal": 2.8e-15, "quadruped_elliptic": 2.9e-14, "quadruped_pyramidal": 3.3e-13}
ESTIMATOR_MEASURED = 1.8e-13                     # EKF (centred, eps = 1e-6); the UKF: 4.2e-17
KIN_BAR = {k: 10 * v for k, v in KIN_MEASURED.items()}
QACC_BAR = {k: 10 * v for k, v in QACC_MEASURED.items()}
TOUCH_BAR = {k: 10 * v for k, v in TOUCH_MEASURED.items()}
ESTIMATOR_BAR = 10 * ESTIMATOR_MEASURED


def _quat(axis, angle):
    a = np.asarray(axis, float)
    return axisangle2quat(a / np.linalg.norm(a), angle)


def _chain3(integrator):
    b = ModelBuilder(timestep=0.005, integrator=integrator)
    off = dict(contype=0, conaffinity=0)
    l1 = b.body("l1", 0, pos=(0, 0, 1.0))
    b.joint(l1, "j1", HINGE, axis=(0, 1, 0), damping=0.05, armature=0.01)
    b.geom(l1, "g1", CAPSULE, size=(0.03, 0), fromto=(0, 0, 0, 0.3, 0, 0), mass=0.5, **off)
    l2 = b.body("l2", l1, pos=(0.3, 0, 0), quat=_quat((1, 0, 1), 0.4))
    b.joint(l2, "j2", HINGE, axis=(0, 0, 1), damping=0.03, armature=0.01)
    b.geom(l2, "g2", CAPSULE, size=(0.025, 0), fromto=(0, 0, 0, 0.25, 0.05, 0), mass=0.3, **off)
    l3 = b.body("l3", l2, pos=(0.25, 0.05, 0), quat=_quat((0, 1, 1), -0.6))
    b.joint(l3, "j3", HINGE, axis=(1, 0, 0), damping=0.02, armature=0.005)
    b.geom(l3, "g3", CAPSULE, size=(0.02, 0), fromto=(0, 0, 0, 0.1, 0, -0.15), mass=0.2, **off)
    b.site(l3, "imu", pos=(0.1, 0.05, -0.02), quat=_quat((1, 2, 3), 0.7))
    for k in (1, 2, 3):
        b.actuator(f"m{k}", f"j{k}", gear=2.0, ctrlrange=(-1, 1), biastype=1, biasprm=(0, 0, -0.05))
    m = b.compile()
    rng = np.random.default_rng(11)
    X = np.concatenate([rng.uniform(-0.8, 0.8, (8, 3)), rng.uniform(-3, 3, (8, 3))], 1)
    X[0, 3:] = 0                                    # one row without velocity
    U = rng.uniform(-0.9, 0.9, (8, 3))
    return m, "imu", [("xbody", "l3"), ("body", "l2")], X, U


def _sphere():
    b = ModelBuilder(timestep=0.002)
    b.geom(0, "floor", PLANE, size=(1, 1, 0.1))
    body = b.body("ball", 0, pos=(0, 0, 1))
    b.joint(body, "f", FREE)
    b.geom(body, "g", SPHERE, size=(0.1,), pos=(0.02, 0, 0.01))
    b.site(body, "imu", pos=(0.05, -0.03, 0.08), quat=_quat((2, -1, 1), 1.1))
    m = b.compile()
    m["disableflags"] = int(m["disableflags"]) | (1 << 4)           # contacts disabled
    rng = np.random.default_rng(12)
    X = np.zeros((8, 13))
    for i in range(8):
        q = rng.standard_normal(4)
        X[i] = np.concatenate([rng.uniform(-0.2, 0.2, 2), [1.0], q / np.linalg.norm(q), rng.uniform(-1, 1, 3), rng.uniform(-6, 6, 3)])
    return m, "imu", [("xbody", "ball"), ("body", "ball")], X, np.zeros((8, 0))


def _filter_arm():
    m, task, mocap, X, U, T = tc.batch("filter_arm", n=8, spread=3.0)
    return m, "tip", [("xbody", int(m["site_bodyid"][m["names"]["site"]["tip"]]))], X, U


def particle_imu_model():
    """the particle (copy-state variant's model) with its tip site turned against the body: accelerometer rows mix the axes"""
    m, task, d = particle(copystate=True)
    m = dict(m)
    sq = np.array(m["site_quat"], float).reshape(-1, 4).copy()
    sq[m["names"]["site"]["tip"]] = (0.5, 0.5, 0.5, 0.5)            # a third of a turn about (1, 1, 1): R permutes the axes, every entry exact
    m["site_quat"] = sq.reshape(np.asarray(m["site_quat"]).shape)
    return m, d


def _particle_imu():
    m, d = particle_imu_model()
    _, _, _, X, U, _ = tc.batch("particle_copystate", n=8, spread=2.0)
    X[0, 2:] = 0; U[0] = 0                           # at rest: qacc = 0 exactly, the accelerometer reads Rᵀ (0, 0, 9.81)
    return m, "tip", [("xbody", "pointmass")], X, U


@functools.lru_cache(maxsize=None)
def kinematic(name):
    """dict(model, task, mocap, X, U, T, site, frames, rows={block name: slice of the residual})"""
    m, site, frames, X, U = {"chain3_euler": lambda: _chain3(0), "chain3_implicitfast": lambda: _chain3(3), "sphere": _sphere,
                             "filter_arm": _filter_arm, "particle_imu": _particle_imu}[name]()
    t = ResidualTable(m); rows = {}

    def block(key, expr):
        rows[key] = slice(t.rows, t.rows + len(expr)); t.sum(expr)
    block("qpos", t.qpos())                                          # an early block in front: the late rows do not start at 0
    block("qacc", t.qacc())
    block("accelerometer", t.accelerometer(site)); block("gyro", t.gyro(site)); block("velocimeter", t.velocimeter(site))
    block("linacc_site", t.linacc("site", site)); block("angacc_site", t.angacc("site", site))
    for ty, b in frames:
        block(f"linacc_{ty}", t.linacc(ty, b)); block(f"angacc_{ty}", t.angacc(ty, b))
    block("qvel", t.qvel())                                          # and one behind
    rows["norm"] = slice(t.rows, t.rows + 1); t.norm(2.0 * t.accelerometer(site) - [0.0, 0.0, 9.81])
    rows["mixed"] = slice(t.rows, t.rows + 1); t.sum(0.5 * t.qacc()[0] - t.gyro(site)[2] + 1.0)
    mocap = np.zeros(7 * m["nmocap"]) if m["nmocap"] else None
    if name == "particle_imu":
        mocap = np.asarray(particle_imu_model()[1]["mocap"], float)
    return dict(model=m, task=t.measurement(), mocap=mocap, X=X, U=U, T=0.05 + 0.1 * np.arange(len(X)), site=site, frames=frames, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- touch
def _twoball(cone):
    b = ModelBuilder(timestep=0.005, cone=cone, impratio=3.0 if cone else 1.0, tolerance=cc.TOLERANCE, iterations=100)
    b.geom(0, "floor", PLANE, size=(2, 2, 0.1), condim=3, friction=(0.8, 0.01, 0.002))
    d = b.body("dumbbell", 0, pos=(0, 0, 0.099))
    b.joint(d, "free", FREE)
    b.geom(d, "left", SPHERE, size=(0.1,), pos=(-0.2, 0, 0), mass=1.0, condim=3)
    b.geom(d, "right", SPHERE, size=(0.1,), pos=(0.2, 0, 0), mass=0.6, condim=4 if cone else 3)
    b.site(d, "one", pos=(-0.2, 0, -0.1), quat=_quat((0, 0, 1), 0.3))          # under the left ball
    b.site(d, "both", pos=(0, 0, -0.1), quat=_quat((0, 1, 0), 0.05))
    m = cc.tighten(b.compile())
    zones = [("one", "sphere", (0.05,)), ("both", "box", (0.3, 0.05, 0.03)), ("both", "capsule", (0.04, 0.1)),
             ("one", "cylinder", (0.06, 0.02)), ("both", "ellipsoid", (0.35, 0.1, 0.04))]
    rng = np.random.default_rng(13)
    q0 = np.concatenate([m["qpos0"], np.zeros(6)])
    X = np.tile(q0, (4, 1))
    X[1:, 0:2] += rng.uniform(-0.3, 0.3, (3, 2)); X[1:, 2] -= rng.uniform(0.0005, 0.002, 3)
    X[1:, 7:10] = rng.uniform(-0.3, 0.3, (3, 3)); X[1:, 12] = rng.uniform(-1, 1, 3)
    return m, zones, X, np.zeros((4, 0)), None


def _quadruped(name):
    """six states of con_cases' rollout of the case (the emulated plan of tests/test_constraint_reference.py: the A1 let go at its
    standing key, 6 to 12 mm over the floor, under seeded controls): steps 4, 8, .. 24 of candidate 0, each with its own control.
    Two or three feet are on the floor in each of them (forces of 1 to 500 N); the front right foot is in the air in the first five"""
    import dyn_cases as dc
    m, task, state, mocap, _ = cc.case(name)
    zones = [(s, FOOT_ZONE[0], FOOT_ZONE[1]) for s, _ in FEET]
    zones += [("FR", "box", (0.05, 0.05, 0.05)), ("FL", "capsule", (0.025, 0.03))]
    N, H = 3, 25
    out = dc.run_emu(m, task, state, mocap, N, H, cc.inputs(name, m, N, H))
    return m, zones, np.array(out["states"][0, 4::4]), np.array(out["actions"][0, 4::4]), mocap


@functools.lru_cache(maxsize=None)
def touch(name):
    """dict(model, task, mocap, X, U, T, zones=[(site id, shape, size)], rows): one residual row per zone behind the qacc block"""
    m, zones, X, U, mocap = _twoball(0 if name.endswith("pyramidal") else 1) if name.startswith("twoball") else _quadruped(name)
    t = ResidualTable(m)
    t.sum(t.qacc())
    for s, shape, size in zones:
        t.sum(t.touch(s, shape, size))
    t.norm(t.touch(zones[0][0], zones[0][1], zones[0][2]) + t.touch(zones[1][0], zones[1][1], zones[1][2]) - 1.0)
    ids = [(m["names"]["site"][s], shape, size) for s, shape, size in zones]
    return dict(model=m, task=t.measurement(), mocap=mocap, X=X, U=U, T=np.zeros(len(X)), zones=ids, nv=m["nv"])


# ---------------------------------------------------------------------------------------------------------------- estimator
def particle_imu_task(m):
    """measurement rows [position (2), accelerometer (3)] of the particle's tip"""
    t = ResidualTable(m)
    t.sum(t.pos("site", "tip"), dim=2); t.sum(t.accelerometer("tip"))
    return t.measurement()


def particle_imu_closed_form(m):
    """A, B of estimator_cases.particle_closed_form; C: position rows [I 0], accelerometer rows Rᵀ ∂(qacc − g)/∂(q, v) with
    qacc = (gear u − damping v) / mass (the x, y slides), so ∂/∂v = −damping / mass on the first two columns of Rᵀ; the control enters
    the accelerometer as D = Rᵀ[:, :2] gear / mass and gravity as the constant Rᵀ (0, 0, 9.81)"""
    import estimator_cases as ec
    from mujoco_mpc_amd.modelgen.builder import quat2mat
    A, B, _ = ec.particle_closed_form(m)
    d = float(np.asarray(m["dof_damping"])[0])
    mass = float(np.asarray(m["body_mass"]).ravel()[-1]) + float(np.asarray(m["dof_armature"])[0]); gear = float(np.asarray(m["actuator_gear"]).ravel()[0])
    R = quat2mat(np.asarray(m["site_quat"], float).reshape(-1, 4)[m["names"]["site"]["tip"]])
    Rt = R.T
    C = np.zeros((5, 4)); C[0, 0] = C[1, 1] = 1.0
    C[2:, 2:4] = -d / mass * Rt[:, :2]
    D = np.zeros((5, 2)); D[2:] = gear / mass * Rt[:, :2]
    y0 = np.zeros(5); y0[2:] = Rt @ np.array([0.0, 0.0, 9.81])
    return A, B, C, D, y0
