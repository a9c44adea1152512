"""Cases of the direct optimiser's window cost (tests/test_direct_cost.py, tests/test_gpu_direct_cost.py; TEST INFRASTRUCTURE ONLY) and the
bars measured on the CPU between the 1-lane emulation and tests/direct_ref.py (none derived from device output).

Every case is a window of direct_ref.Window (hinge dofs, closed-form sensors and forces).  The residual has nr rows; the sensors are the ns
rows from row 1 on, so a row in front of them and rows behind them belong to nobody.  Sensors: a position-stage quadratic one, a
velocity-stage L2 one (dense norm Hessian), an acceleration-stage smooth-abs one (diagonal, not quadratic), and a second position-stage
one; one (t, sensor) pair is masked off in every case.

Why these sizes: T = 3 is the smallest window (one interior configuration whose neighbours are both ends), T = 4 has two interior blocks
that overlap in the band, T = 5 one configuration whose neighbours are both interior.  nv = 3: everything inside one tile; nv = 7 with
ns + nv = 17 rows: one row past the tile, and 21 columns; nv = 18: two chunks of the contraction through LDS, 54 columns, the size of the
quadruped."""
import functools
import os

import numpy as np

import direct_ref as dr

FD_EPS = 1.0e-6          # centred differences of the whole window in direct_ref.Window.jacobian
DIR_EPS = 1.0e-6         # the directional quotient

#                nv  T  settings away from the reference optimiser's defaults
CASES = {
    "nv3_T3": (3, 3, {}),
    "nv3_T4": (3, 4, {}),
    "nv3_T5": (3, 5, {}),
    "nv3_T4_last": (3, 4, dict(last_step_position_sensors=True, last_step_velocity_sensors=True)),
    # the force term alone and unscaled (under h^4 it is 1e-4 of the cost and would hide behind the sensors)
    "nv3_T5_force": (3, 5, dict(sensor_flag=False, time_scaling_force=False)),
    "nv3_T4_unscaled": (3, 4, dict(time_scaling_sensor=False, time_scaling_force=False, first_step_position_sensors=False)),
    "nv7_T4": (7, 4, {}),
    "nv18_T4": (18, 4, dict(time_scaling_force=False)),
}

SENSOR_DIM, SENSOR_STAGE, SENSOR_NORM = [2, 3, 2, 3], [dr.POS, dr.VEL, dr.ACC, dr.POS], [0, 2, 6, 0]
SENSOR_PRM = [[0.0, 0.0], [0.1, 0.0], [0.2, 0.0], [0.0, 0.0]]
FIRST_ROW, NR = 1, 13
H = 0.05


def spec(name):
    nv, T, flags = CASES[name]
    mask = np.ones((T, len(SENSOR_DIM)), int); mask[1, 1] = 0
    rng = np.random.default_rng(11)
    return dr.Spec(nv, NR, H, SENSOR_DIM, SENSOR_STAGE, SENSOR_NORM, SENSOR_PRM, noise_sensor=rng.uniform(0.5, 2.0, len(SENSOR_DIM)),
                   noise_process=rng.uniform(0.5, 2.0, nv), first_row=FIRST_ROW, mask=mask, **flags)


@functools.lru_cache(maxsize=None)
def case(name):
    """the window, what the code under test is given, and the reference (computed once, shared, not to be modified)"""
    nv, T, _ = CASES[name]
    sp = spec(name)
    w = dr.Window(sp, T, seed=100 + sorted(CASES).index(name))
    rs, rf, Df, Ds, V0, V1 = w.inputs()
    ref = w.reference(FD_EPS)
    for v in ref.values():
        v.setflags(write=False)
    return dict(name=name, spec=sp, window=w, T=T, nv=nv, inputs=(rs, rf, *Df, *Ds, V0, V1), ref=ref)


def settings(sp, **override):
    """capi.direct_settings of a direct_ref.Spec"""
    from mujoco_mpc_amd import capi
    kw = dict(sp.flags); kw.update(override)
    return capi.direct_settings(sp.dim, sp.stage, sp.norm_type, sp.prm, sp.noise_sensor, sp.noise_process, sp.h, sensor_first_row=sp.first_row,
                                sensor_mask=sp.mask, **kw)


def deviations(o, ref, T, nv):
    """largest deviation of an output dict from a reference dict, relative to max(1, |entry|): cost, gradient, band, blocks"""
    rel = lambda a, b: float((np.abs(np.asarray(a) - b) / np.maximum(1.0, np.abs(b))).max(initial=0.0))      # noqa: E731
    return dict(cost=rel(o["cost"], ref["cost"]), gradient=rel(o["gradient"], ref["gradient"]), band=rel(o["hessian_band"], ref["hessian_band"]),
                blocks=max(rel(o["block_sensor"], dr.blocks_of(ref["J_s"], T, nv)), rel(o["block_force"], dr.blocks_of(ref["J_f"], T, nv))))


ULP = 2.220446049250313e-16


def bar(table, name, key):
    """ten times the measured deviation; a measurement below one ulp of 1.0 (the unit of a deviation relative to max(1, |entry|)) counts as one
    ulp: the number format cannot show less, and a bar of zero would ask for the reference's bits"""
    return 10.0 * max(table[name][key], ULP)


@functools.lru_cache(maxsize=None)
def algebra_case(name):
    """the case's residuals and blocks with dense seeded velocity blocks (what ball and free joints give), and direct_ref.assemble over them"""
    c = case(name)
    rs, rf, *rest = c["inputs"]
    Df, Ds = rest[0:3], rest[3:6]
    rng = np.random.default_rng(5)
    V0 = np.nan_to_num(rest[6]) + rng.normal(0, 1, rest[6].shape); V1 = np.nan_to_num(rest[7]) + rng.normal(0, 1, rest[7].shape)
    ref = dr.assemble(c["spec"], rs, rf, Df, Ds, V0, V1)
    for v in ref.values():
        v.setflags(write=False)
    return dict(c, inputs=(rs, rf, *Df, *Ds, V0, V1), ref=ref)


# largest deviation of the emulation from direct_ref.Window.reference (whole-window centred differences, eps = FD_EPS), measured on the CPU
# (tests/test_direct_cost.py prints the figures); the bar is ten times the entry
WINDOW_MEASURED = {
    "nv3_T3": dict(cost=5.4e-20, gradient=3.4e-09, band=1.6e-08, blocks=2.0e-07),
    "nv3_T4": dict(cost=3.4e-21, gradient=1.4e-08, band=1.3e-08, blocks=4.9e-08),
    "nv3_T5": dict(cost=0.0, gradient=3.8e-08, band=9.5e-09, blocks=5.8e-07),
    "nv3_T4_last": dict(cost=3.4e-16, gradient=1.9e-08, band=2.9e-08, blocks=9.2e-08),
    "nv3_T5_force": dict(cost=0.0, gradient=9.8e-11, band=1.5e-10, blocks=1.5e-08),
    "nv3_T4_unscaled": dict(cost=0.0, gradient=1.4e-07, band=1.8e-09, blocks=1.9e-08),
    "nv7_T4": dict(cost=4.3e-19, gradient=4.3e-08, band=1.0e-07, blocks=7.8e-08),
    "nv18_T4": dict(cost=0.0, gradient=4.3e-08, band=6.2e-07, blocks=1.4e-07),
}

# the same against direct_ref.assemble (numpy's products over the same blocks, dense seeded velocity blocks)
ALGEBRA_MEASURED = {
    "nv3_T3": dict(cost=5.4e-20, gradient=3.2e-16, band=3.0e-15, blocks=5.6e-16),
    "nv3_T4": dict(cost=3.4e-21, gradient=5.1e-16, band=5.3e-16, blocks=1.3e-15),
    "nv3_T5": dict(cost=0.0, gradient=1.3e-15, band=9.7e-16, blocks=1.3e-15),
    "nv3_T4_last": dict(cost=3.4e-16, gradient=1.8e-15, band=4.8e-16, blocks=4.4e-16),
    "nv3_T5_force": dict(cost=0.0, gradient=1.3e-14, band=2.6e-15, blocks=7.8e-16),
    "nv3_T4_unscaled": dict(cost=0.0, gradient=3.3e-14, band=4.2e-16, blocks=8.0e-16),
    "nv7_T4": dict(cost=4.3e-19, gradient=1.9e-14, band=1.2e-14, blocks=7.1e-15),
    "nv18_T4": dict(cost=0.0, gradient=1.8e-14, band=7.3e-14, blocks=2.1e-14),
}


# ---------------------------------------------------------------------------------------------------------------- a real model
# The 3-hinge chain of inverse_cases (Euler, contact-free, 38 residual rows: positions, velocities, accelerations, IMU rows), T = 3, 4, 5.
# Every named block of its residual is a sensor, its stage the task table's (InverseDerivatives.row_stages); the joint accelerations carry
# the dense L2 norm, the joint velocities the smooth-abs norm, everything else the quadratic one; (t = 1, sensor 2) is masked off.  The
# blocks come from the inverse kernel's finite differences at MODEL_FD_EPS, the reference from whole-window centred differences.
MODEL = "chain3_euler"
MODEL_T = (3, 4, 5)
MODEL_FD_EPS = 1.0e-6          # inverse_cases.FD_EPS


def model_spec(T):
    import inverse_cases as ic
    from mujoco_mpc_amd.derivatives import InverseDerivatives
    c = ic.case(MODEL)
    m, task = c["model"], c["task"]
    rows = sorted(c["late"]["rows"].items(), key=lambda kv: kv[1].start)
    assert rows[0][1].start == 0 and all(a[1].stop == b[1].start for a, b in zip(rows, rows[1:])) and rows[-1][1].stop == task["num_residual"]
    stages = InverseDerivatives(m, task).row_stages()
    dim = [s.stop - s.start for _, s in rows]; stage = [int(stages[s.start]) for _, s in rows]
    assert set(stage) == {dr.POS, dr.VEL, dr.ACC}
    norm = [2 if k == "qacc" else 6 if k == "qvel" else 0 for k, _ in rows]
    mask = np.ones((T, len(dim)), int); mask[1, 2] = 0
    rng = np.random.default_rng(12)
    return dr.Spec(m["nv"], task["num_residual"], float(m["timestep"]), dim, stage, norm, [[0.1, 0.0]] * len(dim), rng.uniform(0.5, 2.0, len(dim)),
                   rng.uniform(0.5, 2.0, m["nv"]), mask=mask, last_step_position_sensors=(T == 4), last_step_velocity_sensors=(T == 4))


MODEL_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct", "chain3_window.npz")
REF_KEYS = ("cost", "gradient", "H", "hessian_band", "J_s", "J_f", "residual_sensor", "residual_force")


def make_model_fixture():
    """the windows' measurements and whole-window references (about half a minute per window: 2 nv T evaluations of the numpy references
    each), written once to tests/golden/ as data; python -c 'import direct_cases; direct_cases.make_model_fixture()' from tests/"""
    import inverse_cases as ic
    out = {}
    for T in MODEL_T:
        w = dr.ModelWindow(model_spec(T), T, ic.case(MODEL), seed=200 + T)
        ref = w.reference(FD_EPS)
        out.update({f"T{T}_Q": w.Q, f"T{T}_y_sensor": w.y_sensor, f"T{T}_y_force": w.y_force})
        out.update({f"T{T}_{k}": ref[k] for k in REF_KEYS})
    np.savez_compressed(MODEL_FIXTURE, **out)


@functools.lru_cache(maxsize=None)
def model_case(T):
    import inverse_cases as ic
    sp = model_spec(T)
    with np.load(MODEL_FIXTURE) as z:
        stored = {k[len(f"T{T}_"):]: z[k] for k in z.files if k.startswith(f"T{T}_")}
    w = dr.ModelWindow(sp, T, ic.case(MODEL), seed=200 + T, stored=stored)
    ref = {k: stored[k] for k in REF_KEYS}
    for v in ref.values():
        v.setflags(write=False)
    return dict(name=f"{MODEL}_T{T}", spec=sp, window=w, T=T, nv=sp.nv, ref=ref)


# largest deviation from direct_ref.ModelWindow.reference of: the emulated inverse evaluations and finite differences
# (tests/emu_inverse_lib.py), then the emulated assemble; measured on the CPU, the bar is ten times the entry
MODEL_MEASURED = {
    "chain3_euler_T3": dict(cost=4.2e-26, gradient=1.5e-13, band=3.9e-08, blocks=5.7e-04),
    "chain3_euler_T4": dict(cost=1.4e-17, gradient=2.3e-13, band=9.1e-08, blocks=2.8e-04),
    "chain3_euler_T5": dict(cost=2.2e-25, gradient=2.5e-12, band=5.4e-07, blocks=1.1e-03),
}
# (the blocks: entries up to 1 / h^2 = 4e4 times a one-sided difference's error; the gradient and the band carry the h^4 weights)


# ---------------------------------------------------------------------------------------------------------------- whole windows on models
# Windows for the window calls (mjpc_hip_direct_cost, mjpc_hip_direct_cost_derivatives) on inverse_cases' models: the 3-hinge chain, the
# free sphere (quaternion dofs, turned by about 0.3 rad per step so the quaternion blocks are far from the identity) and the A1 (nv = 18,
# the compile-time kernel, a free joint and contacts).  q_t = q_{t-1} (+) (h v_0 + seeded tangent noise).
WINDOW_MODELS = {"chain3_euler": 1e-3, "sphere": 0.3, "quadruped_elliptic": 1e-3}
WINDOW_T = 4
# emulation (dc_window_kernel, dc_vblock_kernel) against direct_ref's numpy differentiate_pos and its centred differences over tangent
# nudges (eps = 1e-6), relative to max(1, |entry|), measured on the CPU; the bar is ten times the entry
ROWS_MEASURED = {
    "chain3_euler": dict(velocity=0.0, acceleration=0.0, blocks=2.9e-11),
    "sphere": dict(velocity=2.3e-16, acceleration=4.3e-16, blocks=5.0e-09),
    "quadruped_elliptic": dict(velocity=0.0, acceleration=0.0, blocks=5.1e-09),
}


@functools.lru_cache(maxsize=None)
def window_case(name, T=WINDOW_T):
    """dict(model, task, mocap, Q [T, nq], U [T, nu], time [T], spec, y_sensor, y_force): every run of residual rows of one stage is a sensor,
    norms 0, 2, 6 in turn, (t = 1, sensor 0) masked"""
    import inverse_cases as ic
    from mujoco_mpc_amd.derivatives import InverseDerivatives
    c = ic.case(name)
    m, task = c["model"], c["task"]
    nq, nv, nr, h = m["nq"], m["nv"], task["num_residual"], float(m["timestep"])
    rng = np.random.default_rng(300 + sorted(WINDOW_MODELS).index(name))
    Q = [np.array(c["X"][1][:nq], float)]
    for t in range(1, T):
        Q.append(dr.integrate_pos(m, Q[-1], h * c["X"][1][nq:nq + nv] + WINDOW_MODELS[name] * rng.standard_normal(nv)))
    st = InverseDerivatives(m, task).row_stages()
    cut = [0] + [i for i in range(1, nr) if st[i] != st[i - 1]] + [nr]
    dim = [b - a for a, b in zip(cut, cut[1:])]; stage = [int(st[a]) for a in cut[:-1]]
    mask = np.ones((T, len(dim)), int); mask[1, 0] = 0
    sp = dr.Spec(nv, nr, h, dim, stage, [(0, 2, 6)[i % 3] for i in range(len(dim))], [[0.1, 0.0]] * len(dim), rng.uniform(0.5, 2.0, len(dim)),
                 rng.uniform(0.5, 2.0, nv), mask=mask)
    return dict(name=name, model=m, task=task, mocap=c["mocap"], Q=np.array(Q), U=np.tile(c["U"][1], (T, 1)), time=0.05 + h * np.arange(T), spec=sp,
                y_sensor=rng.normal(0, 0.3, (T, nr)), y_force=rng.normal(0, 0.3, (T, nv)), T=T)


# ---------------------------------------------------------------------------------------------------------------- whole-window references
# The issue's model cases with a dense whole-window reference each (direct_ref.RolloutWindow: inv_ref forces and ref_residual rows, every
# coordinate of every configuration nudged along its tangent, centred, eps = FD_EPS; no chain rule in it), stored as data under
# tests/golden/direct/ because recomputing takes minutes.  The window is a short forward rollout of the emulated step kernel from the
# case's state 1 under its control, each configuration then moved by a seeded 1e-3 tangent noise (rotations of 0.3 rad, where the quaternion
# blocks are far from the identity, are window_case("sphere")'s: there the finite differences of forces of 1e5 N drown the blocks).  InvRef refuses any evaluation within 1e-9 of a contact margin (NearMargin), the window's own and
# every nudged one, so a stored fixture is the assertion that none was.
# Sensors: the sphere's named residual blocks with the task table's stages (dense L2 on the joint accelerations, smooth-abs on the joint
# velocities).  The contact tasks' rows are all acceleration stage by their table (joint accelerations, then touch rows); to have sensors
# of different stages their stages are declared by hand (InverseDerivatives.set_row_stages' notion: a stage decides which of the window's
# ends keep a row, for the code under test and for the reference alike): half of the acceleration rows dense L2 / acceleration, the other
# half quadratic / acceleration, the touch zones smooth-abs / velocity, the last row quadratic / position.  The two-ball case sets
# last_step_position_sensors and last_step_velocity_sensors.  (t = 1, sensor 1) is masked off.
REF_WINDOWS = {"sphere": 1e-3, "twoball_elliptic": 1e-3, "quadruped_elliptic": 1e-3}
REF_T = 4
# the finite-difference mode of the device path, per case (eps = MODEL_FD_EPS): one-sided as the reference optimiser's default, except on the
# A1, where one-sided differences of its elliptic contact forces leave 5e-6 of the gradient (3.0e-04 against a directional truncation of
# 9.0e-08) and centred ones are within it (1.5e-07)
REF_CENTERED = {"sphere": False, "twoball_elliptic": False, "quadruped_elliptic": True}
REF_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct", "{}_window.npz")


def rollout_window(name, T, noise, seed):
    """Q [T, nq], U [T, nu], time [T]: T - 1 emulated steps from the case's state 1, then the tangent noise"""
    import emu_inverse_lib as ei
    import inverse_cases as ic
    c = ic.case(name)
    m, task = c["model"], c["task"]
    nq, h = m["nq"], float(m["timestep"])
    x = np.array(c["X"][1], float); X = [x]
    for t in range(T - 1):
        nxt, _, fail = ei.step_batch(m, task, X[-1][None], c["U"][1][None], [0.05 + h * t], mocap=c["mocap"])
        assert not fail.any()
        X.append(nxt[0])
    rng = np.random.default_rng(seed)
    Q = np.stack([dr.integrate_pos(m, x[:nq], noise * rng.standard_normal(m["nv"])) for x in X])
    return Q, np.tile(c["U"][1], (T, 1)), 0.05 + h * np.arange(T)


def ref_spec(name, T):
    import inverse_cases as ic
    c = ic.case(name)
    m, task = c["model"], c["task"]
    nv, nr, h = m["nv"], task["num_residual"], float(m["timestep"])
    if c["contact"]:
        dim = [nv // 2, nv - nv // 2, nr - nv - 1, 1]; stage = [dr.ACC, dr.ACC, dr.VEL, dr.POS]; norm = [2, 0, 6, 0]
    else:
        from mujoco_mpc_amd.derivatives import InverseDerivatives
        rows = sorted(c["late"]["rows"].items(), key=lambda kv: kv[1].start)
        st = InverseDerivatives(m, task).row_stages()
        dim = [s.stop - s.start for _, s in rows]; stage = [int(st[s.start]) for _, s in rows]
        norm = [2 if k == "qacc" else 6 if k == "qvel" else 0 for k, _ in rows]
    assert sum(dim) == nr and len(set(stage)) == 3 and 2 in norm and 6 in norm
    mask = np.ones((T, len(dim)), int); mask[1, 1] = 0
    rng = np.random.default_rng(13)
    last = name == "twoball_elliptic"
    return dr.Spec(nv, nr, h, dim, stage, norm, [[0.1, 0.0]] * len(dim), rng.uniform(0.5, 2.0, len(dim)), rng.uniform(0.5, 2.0, nv), mask=mask,
                   last_step_position_sensors=last, last_step_velocity_sensors=last)


def _ref_window(name, stored=None):
    import inverse_cases as ic
    seed = 400 + sorted(REF_WINDOWS).index(name)
    Q, U, time = rollout_window(name, REF_T, REF_WINDOWS[name], seed)
    return dr.RolloutWindow(ref_spec(name, REF_T), REF_T, ic.case(name), Q, U, time, seed, stored=stored)


def make_ref_fixture(name):
    """minutes per window; python -c 'import direct_cases; direct_cases.make_ref_fixture(NAME)' from tests/"""
    w = _ref_window(name)
    ref = w.reference(FD_EPS)
    np.savez_compressed(REF_FIXTURE.format(name), Q=w.Q, y_sensor=w.y_sensor, y_force=w.y_force, **{k: ref[k] for k in REF_KEYS})


@functools.lru_cache(maxsize=None)
def ref_case(name):
    with np.load(REF_FIXTURE.format(name)) as z:
        stored = {k: z[k] for k in z.files}
    w = _ref_window(name, stored)
    ref = {k: stored[k] for k in REF_KEYS}
    for v in ref.values():
        v.setflags(write=False)
    c = w.case
    return dict(name=name, spec=w.spec, window=w, T=REF_T, nv=w.spec.nv, ref=ref, model=c["model"], task=c["task"], mocap=c["mocap"], Q=w.Q, U=w.U,
                time=w.time, y_sensor=w.y_sensor, y_force=w.y_force, centered=REF_CENTERED[name])


# emulation of the whole derivative call (window rows and velocity blocks, inverse evaluations and one-sided differences at MODEL_FD_EPS,
# residuals, assemble: tests/test_direct_cost.py::emulated_derivatives) against the stored references, measured on the CPU; bar = ten times
REF_MEASURED = {
    "sphere": dict(cost=4.1e-26, gradient=1.3e-09, band=8.6e-07, blocks=5.7e-02),
    "twoball_elliptic": dict(cost=1.2e-13, gradient=5.7e-07, band=1.1e-06, blocks=1.8e-04),
    "quadruped_elliptic": dict(cost=5.7e-15, gradient=7.4e-07, band=1.6e-03, blocks=2.3e-04),
}
# (entries of the blocks reach 1 / h^2 times a force: 1e6 on the sphere, whose deviation of 6e-2 is 3e-7 of them)
