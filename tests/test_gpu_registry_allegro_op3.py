"""GPU tier of the registry's Allegro and OP3 tasks: the HIP engine at each task's XML shape and at 256 candidates against the oracle
(dynamics) and the independent residual reference tests/task_ref.py (residual rows, costs, returns), the flavour that ran, a forced
spill run bit for bit against the engine's pick, and closed loops through the testspeed harness with the host Transitions."""
import numpy as np
import pytest

import oracle_lib as ol
from mujoco_mpc_amd.modelgen import allegro, op3
from spill_common import chosen_layout
from task_ref import TaskRef

pytestmark = pytest.mark.gpu

TRAJ = ("states", "actions", "times", "residual", "costs", "trace", "knots")
PAIRS = 384          # (candidate, step) pairs whose residual rows are recomputed by task_ref


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _case(name):
    if name == "allegro":
        m, task, d = allegro()
        return m, task, d, d["state"].copy()
    mode = 0 if name == "op3_stand" else 1
    m, task, d = op3(mode=mode)
    st = d["state"].copy()
    st[:m["nq"]] = m["key_qpos"][mode]
    return m, task, d, st


def _engine(m, task, st, N, H, kt, kv, interp, eps, sel):
    from mujoco_mpc_amd.planner import HipBackend
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = be.plan(state=st, mocap=None, time=0.0, knot_times=kt, knot_values=kv, interpolation=interp, num_trajectory=N,
                      horizon=H, sigma=(0.1, 0.0), noise_eps=eps, noise_sel=sel)
        return out, be.fetch_all(N, H, len(kt)), be.lds_bytes(), be.spill_bytes()
    finally:
        be.close()


@pytest.mark.parametrize("name", ["allegro", "op3_stand", "op3_handstand"])
@pytest.mark.parametrize("wide", [False, True], ids=["xml_shape", "n256"])
def test_engine_matches_oracle_dynamics_and_reference_residuals(name, wide, debug_knobs):
    """XML shape (Allegro N 10 / H 51 / P 6, OP3 N 32 / H 24 / P 3, cubic) and 256 candidates: every candidate's states against the
    oracle at the contact models' bar (1e-5), residual rows of PAIRS sampled (candidate, step) pairs against task_ref on the engine's
    own states, costs against the cost table, returns = mean cost, winner = the lowest-index argmin.  Both models run in LDS (no spill slab, the
    flavour mjpc_hip_layout_bytes reports); the same plan forced onto the spill flavour (knob spill = all) is bit-identical."""
    m, task, d, st = _case(name)
    N, H, P = (256 if wide else d["N"]), d["horizon"], d["P"]
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = np.tile(d["ctrl0"], (P, 1))
    eps, sel = ol.noise(11, 0, 0, N, P, m["nu"])
    ref = ol.Oracle(m, task).plan(st, None, 0.0, kt, kv, d["interp"], N, H, sigma=(0.1, 0.0), noise_eps=eps, noise_sel=sel, nthreads=8)
    out, allc, lds, slab = _engine(m, task, st, N, H, kt, kv, d["interp"], eps, sel)
    want = chosen_layout(m, task)
    assert slab == 0 and not want[2] and lds == want[0]              # the in-LDS flavour the host-only query names
    assert np.array_equal(out["failure"], ref["failure"]) and not out["failure"].any()
    assert np.array_equal(allc["knots"], ref["knots"]) and np.array_equal(allc["times"], ref["times"])
    assert _rel(allc["actions"], ref["actions"]) < 1e-14
    assert _rel(allc["states"], ref["states"]) < 1e-5
    if task["num_trace"]:
        assert _rel(allc["trace"], ref["trace"]) < 1e-5
    assert allc["diag"][:, 1].max() >= 1
    tr = TaskRef(m, task)
    rng = np.random.default_rng(5)
    k = rng.choice(N * H, min(PAIRS, N * H), replace=False)
    c, t = k // H, k % H
    nq, nv = m["nq"], m["nv"]
    S = allc["states"][c, t]
    r = tr.residual(S[:, :nq], S[:, nq:nq + nv], allc["actions"][c, t])
    assert _rel(allc["residual"][c, t], r) < 1e-10
    assert _rel(allc["costs"], tr.cost(allc["residual"])) < 1e-12
    assert _rel(out["returns"], allc["costs"].mean(1)) < 1e-12
    assert out["winner"] == int(np.argmin(out["returns"]))              # (the oracle writes no residual rows for ids 17 / 18: no winner there)
    # the spill flavour, forced, computes the same bits
    debug_knobs("spill", "all")
    out2, allc2, lds2, slab2 = _engine(m, task, st, N, H, kt, kv, d["interp"], eps, sel)
    assert slab2 > 0 and lds2 < lds
    assert np.array_equal(out["returns"], out2["returns"]) and out["winner"] == out2["winner"]
    for key in TRAJ:
        assert np.array_equal(allc[key], allc2[key]), key


def test_closed_loop_allegro_and_its_transition():
    """testspeed loop on the Allegro task (allegro.cc): planning with the task's numerics (6 cubic spline points, exploration 0.1,
    32 trajectories) keeps the cube on the hand over 40 steps instead of on the floor at z = -0.2 + 0.03; Allegro::TransitionLocked
    (allegro.cc:79-110) puts a cube that lies still on the floor back to its qpos0 pose.  Measured on an MI355X: the cube ends at
    z 0.045 (bar -0.05, the floor rest height is -0.17); the reset cube ends at (0.258, 0.012, 0.044) after rolling on the fingers,
    0.058 / 0.012 from qpos0 in x / y (bars 0.1, where the floor pose was 0.25 / 0.2 away) and above the bar z -0.1."""
    from mujoco_mpc_amd import cplanner
    m, task, d = allegro()
    num = dict(sampling_spline_points=6, sampling_exploration=0.1, sampling_trajectories=32, sampling_representation=2)
    p = cplanner.SamplingPlanner()
    p.Initialize(m, task, num, max_samples=32, max_horizon=51)
    p.Reset(51, d["ctrl0"])                                          # initial repeated action: the home key's servo targets
    res = cplanner.testspeed(p, d["state"], None, horizon=51, steps_per_planning_iteration=1, total_time=40 * m["timestep"])
    print("allegro closed loop: cube z", res["state"][6], "average cost", res["average_cost"])
    assert not res["failure"] and res["state"][6] > -0.05 and np.isfinite(res["average_cost"])
    st = d["state"].copy()
    st[4:7] = [0.45, 0.2, -0.2 + 0.03]; st[7:11] = [1, 0, 0, 0]      # at rest on the floor, 0.25 / 0.2 away from qpos0 in x / y
    res = cplanner.testspeed(p, st, None, horizon=51, steps_per_planning_iteration=1, total_time=30 * m["timestep"])
    print("allegro reset: cube", res["state"][4:7], "qpos0", m["qpos0"][4:7])
    assert abs(res["state"][4] - m["qpos0"][4]) < 0.1 and abs(res["state"][5] - m["qpos0"][5]) < 0.1 and res["state"][6] > -0.1
    p.close()


def test_closed_loop_op3_stand_and_the_mode_transition():
    """testspeed loop on OP3 (stand.cc) with the task's numerics (3 cubic spline points, exploration 0.1, 32 trajectories):
    Stand from the home key keeps the torso upright over 1.5 s; a run asked for mode 1 from the start has OP3::TransitionLocked
    (stand.cc:154-163) install the Handstand height goal 0.57 (kModeHeight, stand.h:61), while Stand keeps 0.38.  Measured on an
    MI355X: the torso's z axis ends at z 0.998 (bar 0.9) and body_link at 0.241 m (bar 0.2; 0.246 at the home key)."""
    from mujoco_mpc_amd import cplanner
    m, task, d = op3()
    num = dict(sampling_spline_points=3, sampling_exploration=0.1, sampling_trajectories=32, sampling_representation=2)
    res = {}
    for mode in (0, 1):
        p = cplanner.SamplingPlanner()
        p.Initialize(m, task, num, max_samples=32, max_horizon=24)
        p.Reset(24, d["ctrl0"])
        res[mode] = cplanner.testspeed(p, d["state"], None, horizon=24, steps_per_planning_iteration=1, total_time=1.5, mode=mode, mode_time=0.0)
        p.close()
        assert not res[mode]["failure"]
    q = res[0]["state"][3:7]
    upright = 1 - 2 * (q[1] ** 2 + q[2] ** 2)                        # z component of the torso's z axis
    print("op3 stand: torso height", res[0]["state"][2], "upright", upright, "average cost", res[0]["average_cost"],
          "parameters", res[0]["parameters"], res[1]["parameters"])
    assert upright > 0.9 and res[0]["state"][2] > 0.2
    assert res[0]["parameters"][0] == 0.38 and res[1]["parameters"][0] == 0.57
