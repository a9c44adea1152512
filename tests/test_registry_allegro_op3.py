"""CPU tier of the registry's Allegro and OP3 tasks (MJPC_TASK_ALLEGRO = 17, MJPC_TASK_OP3 = 18): the kernel source in its 1-lane
emulation against the oracle for the dynamics, and against the independent residual reference tests/task_ref.py for the residual
rows, costs and returns (oracle/task.c has no case for these ids); quirk pins; the generators against the task files
(tests/golden/mjcf/allegro_op3.npz); the ABI values and the host-only layout query."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
import oracle_lib as ol
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.modelgen import REGISTRY, allegro, op3
from mujoco_mpc_amd.modelgen.tasks import OP3_MODE_HEIGHT
from task_ref import TaskRef, _t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _case(name):
    """(model, task, defaults, start state): Allegro from its home key, OP3 Stand from `home`, OP3 Handstand from `handstand`"""
    if name == "allegro":
        m, task, d = allegro()
        return m, task, d, d["state"].copy()
    mode = 0 if name == "op3_stand" else 1
    m, task, d = op3(mode=mode)
    st = d["state"].copy()
    st[:m["nq"]] = m["key_qpos"][mode]
    return m, task, d, st


def _plan(name, N=6, sigma=0.1, seed=1):
    """the task's own P, H and spline; nominal = the servo targets of the key, explicit Philox noise"""
    m, task, d, st = _case(name)
    P, H = d["P"], d["horizon"]
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.tile(d["ctrl0"], (P, 1))
    eps, sel = ol.noise(seed, 0, 0, N, P, m["nu"])
    args = (st, None, 0.0, kt, kv, d["interp"], N, H)
    a = ol.Oracle(m, task).plan(*args, sigma=(sigma, 0.0), noise_eps=eps, noise_sel=sel, nthreads=4)
    b = emu_lib.plan(m, task, *args, sigma=(sigma, 0.0), noise_eps=eps, noise_sel=sel)
    return m, task, a, b


def _ref_rows(m, task, out):
    nq, nv = m["nq"], m["nv"]
    S = out["states"].reshape(-1, out["states"].shape[-1]); A = out["actions"].reshape(-1, m["nu"])
    tr = TaskRef(m, task)
    r = tr.residual(S[:, :nq], S[:, nq:nq + nv], A).reshape(out["residual"].shape)
    return tr, r


NAMES = ["allegro", "op3_stand", "op3_handstand"]


@pytest.mark.parametrize("name", NAMES)
def test_kernel_source_dynamics_match_the_oracle_and_residuals_the_reference(name):
    """Dynamics against the oracle at the bars test_kernel_source_matches_oracle uses for colliders of these classes (box / sphere /
    capsule / convex mesh against planes and boxes: 1e-5); residuals, costs and returns against task_ref only."""
    m, task, a, b = _plan(name)
    assert a["unsupported"] == 0 and not a["failure"].any() and not b["failure"].any()
    assert np.array_equal(a["knots"], b["knots"]) and np.array_equal(a["times"], b["times"]) and np.array_equal(a["actions"], b["actions"])
    assert _rel(b["states"], a["states"]) < 1e-5
    if task["num_trace"]:
        assert _rel(b["trace"], a["trace"]) < 1e-5
    assert b["diag"][:, 1].max() >= 1                     # contacts are in play (cube on the hand / feet or forearms on the floor)
    tr, r = _ref_rows(m, task, b)
    assert _rel(b["residual"], r) < 1e-12
    assert _rel(b["costs"], tr.cost(r)) < 1e-12
    assert _rel(b["returns"], tr.cost(r).mean(1)) < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_residual_rows_costs_returns_and_winner(name):
    """Every candidate and step: residual rows against task_ref at 1e-12 relative on the emulated kernel's own states, costs against
    the cost table (mjpc/norm.cc), returns = the mean of the costs, winner = the lowest-index argmin of the returns."""
    m, task, _, b = _plan(name, N=8, sigma=0.2, seed=3)
    tr, r = _ref_rows(m, task, b)
    nr = int(task["num_residual"])
    assert b["residual"].shape[-1] == nr == (57 if name == "allegro" else 53)
    err = np.abs(b["residual"] - r).max((0, 1)) / (np.abs(r).max() + 1e-300)
    assert err.max() < 1e-12, (int(err.argmax()), float(err.max()))
    c = tr.cost(b["residual"])
    assert _rel(b["costs"], c) < 1e-12
    ret = b["costs"].mean(1)
    assert _rel(b["returns"], ret) < 1e-12
    assert int(np.argmin(b["returns"])) == int(np.flatnonzero(b["returns"] == b["returns"].min())[0])
    assert np.ptp(b["returns"]) > 0                      # the candidates differ


def _one_step(m, task, state, ctrl, actions=False):
    """residual of a single-step rollout at `state` (the first row is the state handed in); actions=True: also the action the
    planner applied (ctrl clamped to the control range)"""
    kt = np.array([0.0]); kv = ctrl[None, :]
    out = emu_lib.plan(m, task, state, None, 0.0, kt, kv, 0, 1, 2, sigma=(0.0, 0.0))
    return (out["residual"][0, 0], out["actions"][0, 0]) if actions else out["residual"][0, 0]


def test_allegro_quirk_grasp_slice_covers_the_cube_quaternion():
    """allegro.cc:64-66: qpos[7:23] - key_qpos[7:23] starts inside the cube's free joint (the goal's ball joint comes first), so a
    change of the cube's quaternion alone moves rows 25-28; rows 29-40 (hand joints 0-11) and the other slices' widths stay put."""
    m, task, d, st = _case("allegro")
    r0 = _one_step(m, task, st, d["ctrl0"])
    s1 = st.copy()
    s1[7:11] = [np.cos(0.2), 0.0, 0.0, np.sin(0.2)]
    r1 = _one_step(m, task, s1, d["ctrl0"])
    moved = np.abs(r1 - r0) > 1e-12
    assert moved[25:29].any() and not moved[29:41].any()
    assert np.allclose(r1[25:29], s1[7:11] - m["key_qpos"][0][7:11], rtol=0, atol=1e-15)
    assert moved[3:6].any()                               # subQuat(goal, cube) sees it too
    tr = TaskRef(m, task)
    assert _rel(r1, tr.residual(s1[None, :27], s1[None, 27:], d["ctrl0"][None])[0]) < 1e-12


def test_op3_handstand_quirk_lifting_the_left_hand_lowers_the_height_row():
    """stand.cc:64-67: 0.5 (l_foot_z + r_foot_z) - 0.5 (l_hand_z - r_hand_z): a minus between the hands, so raising the left hand
    alone LOWERS the height residual (with a plus it would raise it).  The left hand is raised by its shoulder roll."""
    m, task, d, st = _case("op3_handstand")
    tr = TaskRef(m, task)
    lh = int(task["int_data"][4])
    qa = m["jnt_qposadr"][m["names"]["joint"]["l_sho_roll"]]
    nq = m["nq"]
    z0 = tr.ref.fk(_t(st[None, :nq]))["site_xpos"][0, lh, 2].item()
    best = None
    for dq in (0.3, -0.3):
        s1 = st.copy(); s1[qa] += dq
        z1 = tr.ref.fk(_t(s1[None, :nq]))["site_xpos"][0, lh, 2].item()
        if z1 > z0 + 1e-3:
            best = s1
            break
    assert best is not None
    r0 = _one_step(m, task, st, d["ctrl0"]); r1, u = _one_step(m, task, best, d["ctrl0"], actions=True)
    assert r1[0] < r0[0] - 1e-4
    assert _rel(r1, tr.residual(best[None, :nq], best[None, nq:], u[None])[0]) < 1e-12


def test_op3_stand_upright_tail_is_exactly_zero():
    """stand.cc:117-118: in Stand the last six of the 13 upright rows (29-34) are written as zeros, whatever the state."""
    m, task, a, b = _plan("op3_stand", N=4, sigma=0.3)
    assert np.all(b["residual"][..., 29:35] == 0.0)
    assert np.abs(b["residual"][..., 22:29]).max() > 0
    m1, task1, a1, b1 = _plan("op3_handstand", N=4, sigma=0.3)
    assert np.abs(b1["residual"][..., 29:35]).max() > 0     # in Handstand the same rows carry the feet's and the torso's axes


@pytest.mark.parametrize("mode", [0, 1])
def test_op3_nominal_control_rows_follow_the_key_of_the_mode(mode):
    """stand.cc:92-95: ctrl - key_qpos[nq * mode + 7 : + nu]; the same controls price against the home key in Stand and against the
    handstand key in Handstand."""
    m, task, d = op3(mode=mode)
    ctrl = np.asarray(m["key_qpos"][0][7:25], float) + 0.01 * np.arange(18)
    r = _one_step(m, task, d["state"], ctrl)
    np.testing.assert_array_equal(r[4:22], ctrl - m["key_qpos"][mode][7:25])
    assert float(task["parameters"][0]) == OP3_MODE_HEIGHT[mode] and int(task["int_data"][0]) == mode


# ----------------------------------------------------------------------------------- the generators against the task files
def _fixture():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_allegro_op3_fixtures as mk
    return mk.load()


def _check_common(fx, m, task, d, traces):
    info = fx["info"]
    terms = info["cost_terms"]
    assert [int(t[0]) for t in terms] == list(task["dim_norm_residual"])
    assert [int(t[1]) for t in terms] == list(task["norm"])
    np.testing.assert_array_equal([float(t[2]) for t in terms], task["weight"])
    np.testing.assert_array_equal([p for t in terms for p in t[3]], task["norm_parameter"])
    num = info["numeric"]
    assert m["timestep"] == num["agent_timestep"][0]
    assert d["horizon"] == int(num["agent_horizon"][0] / num["agent_timestep"][0] + 1)           # agent.cc:107
    assert d["P"] == int(num["sampling_spline_points"][0]) and d["N"] == int(num["sampling_trajectories"][0])
    assert d["interp"] == int(num.get("sampling_representation", [2])[0])                        # kCubicSpline by default
    assert d["sigma"][0] == num["sampling_exploration"][0]
    keys = info["keys"]
    assert m["nkey"] == len(keys)
    for k, key in enumerate(keys):
        np.testing.assert_array_equal(m["key_qpos"][k], key["qpos"])
        assert m["names"]["key"][key["name"]] == k
    bn = {v: k for k, v in m["names"]["body"].items()}
    assert [("body", bn[int(i)]) for i in task["trace_objid"]] == traces
    assert all(int(t) == 1 for t in task["trace_objtype"])


def test_allegro_generator_matches_the_task_file():
    fx = _fixture()["allegro"]
    m, task, d = allegro()
    _check_common(fx, m, task, d, [tuple(t) for t in fx["info"]["traces"]] + [tuple(t) for t in fx["traces"]])
    assert [t[1] for t in fx["traces"]] == ["rf_tip", "ff_tip", "mf_tip", "th_tip"]
    assert fx["option"] == dict(integrator="implicitfast", iterations="100", ls_iterations="50")
    assert m["integrator"] == 3 and m["iterations"] == 100 and m["ls_iterations"] == 50
    bid = m["names"]["body"]
    for b in fx["bodies"][1:]:
        np.testing.assert_allclose(m["body_pos"][bid[b["name"]]], b["pos"], rtol=0, atol=1e-15)
    palm = bid["palm"]
    np.testing.assert_allclose(m["body_pos"][palm], fx["palm"]["pos"], rtol=0, atol=0)
    q = np.array(fx["palm"]["quat"]); np.testing.assert_allclose(m["body_quat"][palm], q / np.linalg.norm(q), rtol=0, atol=1e-15)
    assert np.all(m["actuator_gainprm"][:, 0] == fx["kp"]) and np.all(m["actuator_biasprm"][:, 1] == -fx["kp"])
    sid = m["names"]["site"]
    assert m["site_bodyid"][sid["grasp_site"]] == palm and np.all(m["site_pos"].reshape(-1, 3)[sid["grasp_site"]] == fx["sites"]["grasp_site"])
    assert list(task["int_data"]) == [sid["grasp_site"], bid["cube"], bid["goal"], 0]
    sensors = {s["name"]: s for s in fx["info"]["sensors"]}
    assert sensors["cube_goal_position"]["objname"] == "grasp_site" and sensors["cube_goal_orientation"]["objname"] == "goal"


def test_op3_generator_matches_the_task_file():
    fx = _fixture()["op3"]
    for mode in (0, 1):
        m, task, d = op3(mode=mode)
        _check_common(fx, m, task, d, [])
        assert (m["nq"], m["nv"], m["nu"]) == (25, 24, 18)
        assert fx["removed_joints"] == ["head_pan", "head_tilt"] and not set(fx["removed_joints"]) & set(m["names"]["joint"])
        assert not {a[:-4] for a in fx["removed_actuators"]} & {a[:-4] for a in m["names"]["actuator"]}
        assert fx["info"]["numeric"]["residual_Height Goal"][0] == OP3_MODE_HEIGHT[0]
        assert fx["info"]["text"]["task_transition"] == "Stand|Handstand"
        sid = m["names"]["site"]
        sp = m["site_pos"].reshape(-1, 3)
        for name, pos in fx["sites"].items():
            np.testing.assert_array_equal(sp[sid[name]], pos)
        boxes = sorted((tuple(m["geom_pos"][g]), tuple(m["geom_size"][g])) for g in range(m["ngeom"]) if m["geom_type"][g] == 6
                       and m["geom_bodyid"][g] in (m["names"]["body"]["l_ank_roll_link"], m["names"]["body"]["r_ank_roll_link"]))
        assert boxes == sorted((tuple(p), tuple(s)) for p, s in fx["feet"])
        sensors = {s["name"]: s for s in fx["info"]["sensors"]}
        I = list(task["int_data"])
        assert I[:7] == [mode] + [sid[sensors[n]["objname"]] for n in ("head_position", "left_foot_position", "right_foot_position",
                                                                        "left_hand_position", "right_hand_position", "torso_up")]
        assert I[7] == m["names"]["body"][sensors["body_subtreecom"]["body"]]
        assert np.any(m["geom_type"] == 7)                   # the forearms are convex meshes
        np.testing.assert_array_equal(d["ctrl0"], m["key_qpos"][mode][7:25])


# ----------------------------------------------------------------------------------- ABI
def test_task_enum_values_in_the_header():
    with open(os.path.join(ROOT, "include", "mjpc_hip.h")) as f:
        h = f.read()
    assert re.search(r"MJPC_TASK_ALLEGRO\s*=\s*17\b", h) and re.search(r"MJPC_TASK_OP3\s*=\s*18\b", h)
    assert REGISTRY["allegro"]()[1]["task_id"] == 17 and REGISTRY["op3"]()[1]["task_id"] == 18


# per-flavour layout bytes (host-only query), recorded: LDS bytes of the cached (model tables in LDS) and direct flavours, and
# the flavour / slab mjpc_hip_create picks.  Both fit LDS without the spill tier.
LAYOUT = {"allegro": dict(cached=149040, direct=134072), "op3": dict(cached=148344, direct=134968)}


@pytest.mark.parametrize("name", ["allegro", "op3"])
def test_layout_bytes_per_flavour(name):
    lib = C.CDLL(capi.ENGINE_PATH)
    lib.mjpc_hip_layout_bytes.argtypes = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), C.c_int]
    lib.mjpc_hip_debug_spill_layout.argtypes = [C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    m, task, _ = REGISTRY[name]()
    cm = capi.CModel(m, task)
    got = {k: lib.mjpc_hip_layout_bytes(C.byref(cm.c_model), C.byref(cm.c_task), v) for k, v in (("cached", 1), ("direct", 0))}
    a = C.c_int(0); b = C.c_int(0)
    rc = lib.mjpc_hip_debug_spill_layout(C.byref(cm.c_model), C.byref(cm.c_task), C.byref(a), C.byref(b))
    assert rc == 0 and b.value == 0 and 0 < a.value <= LDS_LIMIT          # the engine picks an in-LDS flavour: no spill tier
    assert 0 < got["direct"] <= LDS_LIMIT
    want = LAYOUT[name]
    for k, v in want.items():
        if v is not None:
            assert got[k] == v, (k, got[k], v)
