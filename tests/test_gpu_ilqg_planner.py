"""GPU tier of the iLQG planner (mjpc_hip::iLQGPlanner through cplanner.iLQGPlanner): the C++ planner against the numpy mirror of the
planner loop on HipBackend in closed loop on the particle, the reference's iLQGTest.Particle, BestRollout's tie, the all-failed branch of
NominalTrajectory, the early return on a failed backward pass, and the testspeed harness with planner kind 4."""
import ctypes as C

import numpy as np
import pytest

import feedback_cases as fc
import ilqg_planner_mirror as im
from mujoco_mpc_amd import capi, cplanner
from mujoco_mpc_amd import derivatives as D
from mujoco_mpc_amd.modelgen import particle, quadruped
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu


def _hip_mirror(m, task, mocap, be, H, N, rep=1):
    def rollouts(state, time, Hh, pol, mode, r, alpha, scale, improvement):
        o = be.plan_feedback(state, time, Hh, pol["times"], pol["states"], pol["actions"], pol["K"], alpha, scale,
                             action_improvement=pol["k"] if improvement else None, mode=mode, representation=r, mocap=mocap)
        return dict(returns=o["returns"], failure=o["failure"], rows=lambda i: be.candidate(i, Hh, 0))

    def backward(x, u, t, res, reg, rate):
        return be.trajectory_ilqg(x, u, t, res, mocap=mocap, eps=1e-6, centered=False, regularization=reg, regularization_rate=rate)
    return im.ILQGPlannerMirror(m, rollouts, backward, H, N, rep)


def test_cpp_ilqg_planner_matches_the_mirror_in_closed_loop_on_the_particle():
    """six plan steps with the world stepped between them; per plan step the line-search steps, the winner, action_step, feedback_scaling and
    the regularisation are equal, the returns agree at 1e-9, the adopted policy's actions, gains and improvement are bit-equal, and so is
    ActionFromPolicy (with and without a state; use_previous returns the earlier policy)"""
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H, N = 16, 8
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    world = HipBackend(m, task, max_samples=1, max_horizon=2)
    mir = _hip_mirror(m, task, mocap, be, H, N)
    cpp = cplanner.iLQGPlanner()
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=N, ilqg_representation=1), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    x = np.array([0.3, -0.2, 0.0, 0.0]); t = 0.0
    first = last = None
    for it in range(6):
        cpp.SetState(x, mocap, None, t); cpp.OptimizePolicy(H)
        mir.set_state(x, t); mir.optimize(H)
        v = cpp.values()
        assert not v["backward_pass_failed"] and not mir.backward_failed and not v["all_failed"], it
        assert np.array_equal(cpp.linesearch_steps(), mir.steps), it
        r = cpp.returns(N)
        assert np.abs(r - mir.returns).max() <= 1e-9 * max(1.0, np.abs(mir.returns).max()), it
        assert v["winner"] == mir.winner and v["action_step"] == mir.action_step and v["feedback_scaling"] == mir.feedback_scaling, it
        assert v["regularization"] == mir.reg and v["regularization_rate"] == mir.rate, it
        assert abs(v["improvement"] - mir.improvement) <= 1e-9 and abs(v["surprise"] - mir.surprise) <= 1e-6, it
        p = cpp.get_policy(0)
        assert p["horizon"] == H and p["feedback_scaling"] == 1.0
        assert np.array_equal(p["actions"], mir.policy["actions"][:H]), it
        assert np.array_equal(p["feedback_gain"], mir.policy["K"][:H]) and np.array_equal(p["action_improvement"], mir.policy["k"][:H]), it
        assert np.array_equal(p["times"], mir.policy["times"][:H]) and np.array_equal(p["states"], mir.policy["states"][:H]), it
        for tq in (t, t + 0.05, t + 0.7):
            for st in (None, x + 0.01):
                a = cpp.ActionFromPolicy(tq, state=st)
                assert np.array_equal(a, D.ilqg_policy_action(m, p["times"], p["states"], p["actions"], p["feedback_gain"], tq, st, 1, feedback_scaling=1.0)), (it, tq)
                with fc.summation_rule():          # riccati_mirror.policy_action with its gain product by the summation rule
                    assert np.array_equal(a, mir.action(tq, st, H=H)), (it, tq)
                assert np.abs(a - mir.action(tq, st, H=H)).max() <= 1e-14          # and with numpy's own product
        if it > 0:
            q = cpp.get_policy(1)
            assert np.array_equal(q["actions"], prev["actions"]) and np.array_equal(q["feedback_gain"], prev["feedback_gain"])
            assert np.array_equal(cpp.ActionFromPolicy(t, use_previous=True, state=x),
                                  D.ilqg_policy_action(m, prev["times"], prev["states"], prev["actions"], prev["feedback_gain"], t, x, 1, feedback_scaling=1.0))
        prev = p
        best = cpp.BestTrajectory()
        assert best.horizon == H and np.abs(best.states - mir.best["states"]).max() < 1e-9
        first = first if first is not None else best.total_return
        last = best.total_return
        for _ in range(2):                                          # the world moves two steps under the new policy, with feedback
            u = cpp.ActionFromPolicy(t, state=x)
            o = world.step_batch(x[None], u[None], np.array([t]), mocap=mocap)
            x = o["next_states"][0]; t += 0.1
    assert last < first
    be.close(); world.close()


def test_reference_ilqg_test_particle():
    """mjpc/test/ilqg_planner/ilqg_test.cc: timestep 0.1, 26 steps, 25 OptimizePolicy calls from the same state; the nominal's final
    position within 1e-2 of the goal, its final velocity within 1e-1, every nominal action inside the ctrlrange"""
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H = 26
    cpp = cplanner.iLQGPlanner()
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=10), max_samples=16, max_horizon=H)
    cpp.Reset(H)
    x = np.asarray(d["state"], float)
    cpp.SetState(x, mocap, None, 0.0)
    for _ in range(25):
        cpp.OptimizePolicy(H)
    best = cpp.BestTrajectory()
    goal = mocap[:2]
    print("final position error", np.abs(best.states[H - 1, :2] - goal), "final velocity", best.states[H - 1, 2:4])
    assert np.abs(best.states[H - 1, :2] - goal).max() <= 1e-2
    assert np.abs(best.states[H - 1, 2:4]).max() <= 1e-1
    cr = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2)
    assert np.all(best.actions >= cr[:, 0]) and np.all(best.actions <= cr[:, 1])


def test_best_rollout_ties_and_failures():
    assert cplanner.ilqg_best_rollout([1.0, 1.0, 1.0, 1.0], [0, 0, 0, 0]) == 3           # all equal: the highest index
    assert cplanner.ilqg_best_rollout([1.0, 0.5, 0.5, 2.0], [0, 0, 0, 0]) == 2
    assert cplanner.ilqg_best_rollout([1.0, 0.5, 0.5, 2.0], [0, 0, 1, 0]) == 1
    assert cplanner.ilqg_best_rollout([0.1, 0.5], [1, 1]) == -1
    assert im.best_rollout([1.0, 1.0, 1.0], [0, 0, 0]) == 2 and im.best_rollout([1.0], [1]) == -1


def test_all_equal_steps_pick_the_highest_index_and_all_failed_takes_the_reference_branch():
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H, N = 8, 4
    cpp = cplanner.iLQGPlanner()
    # min_linesearch_step = 1: every step but the last is 1, the policy has zero gains: candidates 0 .. N-2 are the same rollout, and the
    # last (scale 0) as well: a four-way tie
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=N), settings=dict(min_linesearch_step=1.0), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    x = np.asarray(d["state"], float)
    cpp.SetState(x, mocap, None, 0.0)
    cpp.NominalTrajectory(H)
    r = cpp.returns(N)
    assert np.all(r == r[0])
    v = cpp.values()
    assert v["feedback_scaling"] == 0.0 and not v["all_failed"]          # the winner is index N-1, whose step is 0
    # a NaN state fails every candidate: the reference's branch keeps the policy's trajectory and zeroes the feedback scaling
    before = cpp.get_policy(0)
    bad = x.copy(); bad[0] = np.nan
    cpp.SetState(bad, mocap, None, 0.0)
    cpp.NominalTrajectory(H)
    v = cpp.values()
    assert v["all_failed"] and v["feedback_scaling"] == 0.0
    c = cpp.get_policy(2)
    assert np.array_equal(c["states"], before["states"]) and np.array_equal(c["actions"], before["actions"])


def test_failed_backward_pass_returns_early_with_the_policy_unchanged():
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H, N = 8, 4
    cpp = cplanner.iLQGPlanner()
    # max_regularization_iterations = 0: the regularisation loop never runs a sweep, so the pass reports failure (planner.cc:429-431, 524)
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=N), settings=dict(max_regularization_iterations=0), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    cpp.SetState(np.asarray(d["state"], float), mocap, None, 0.0)
    before = cpp.get_policy(0)
    cpp.OptimizePolicy(H)
    v = cpp.values()
    print("backward pass failed:", v["backward_pass_failed"], "winner", v["winner"])
    assert v["backward_pass_failed"] and v["winner"] == -1
    after = cpp.get_policy(0)
    for k in ("actions", "feedback_gain", "action_improvement"):
        assert np.array_equal(before[k], after[k]), k
    assert cpp.BestTrajectory() is None or cpp.BestTrajectory().horizon == 0


def test_out_of_range_horizon_is_refused_and_leaves_the_policy_unchanged():
    """OptimizePolicy with a horizon beyond max_horizon, below 2, or with an empty batch: NominalTrajectory refuses (PlannerError for the
    horizon), Iteration is not entered, nothing of the policy changes - also on the very first call, when no line-search steps exist yet -
    and the planner still works afterwards; Iteration on its own, without a nominal trajectory of that horizon, is refused as well"""
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H, N = 8, 4
    cpp = cplanner.iLQGPlanner()
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=N), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    cpp.SetState(np.asarray(d["state"], float), mocap, None, 0.0)
    before = cpp.get_policy(0)
    for bad in (H + 1, 4 * H, 1, 0):
        with pytest.raises(cplanner.PlannerError):
            cpp.OptimizePolicy(bad)
        after = cpp.get_policy(0)
        for k in ("times", "states", "actions", "feedback_gain", "action_improvement"):
            assert np.array_equal(before[k], after[k]), (bad, k)
        assert cpp.values()["winner"] == -1
    cpp.set_num_trajectory(0)
    cpp.OptimizePolicy(H)                                # an empty batch: the reference returns without rolling anything out
    assert cpp.values()["winner"] == -1 and np.array_equal(cpp.get_policy(0)["actions"], before["actions"])
    cpp.set_num_trajectory(N)
    cpp.OptimizePolicy(H)
    assert cpp.values()["winner"] >= 0 and not cpp.values()["backward_pass_failed"]
    cpp.NominalTrajectory(H)
    with pytest.raises(cplanner.PlannerError):
        cpp.Iteration(H - 1)


def test_testspeed_kind_4_runs_the_a1():
    m, task, d = quadruped()
    cm = capi.CModel(m, task)
    H, N = 12, 8
    cpp = cplanner.iLQGPlanner()
    cpp.Initialize(m, task, dict(ilqg_num_rollouts=N), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    state = np.ascontiguousarray(d["state"], float).copy(); mocap = np.ascontiguousarray(d["mocap"], float).copy()
    out = np.zeros(6)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)          # noqa: E731
    total = cplanner.lib().mjpc_testspeed_run(C.byref(cm.c_model), C.byref(cm.c_task), cpp._h, 4, dp(state), dp(mocap) if mocap.size else None, 0.0, H, 4,
                                              float(m["timestep"]) * 12, 0, None, dp(out), 0, 0.0, None)
    cplanner._check()
    print("testspeed kind 4: total cost", total, "plan steps", out[4], "failure", out[5])
    assert out[5] == 0 and out[4] >= 3 and np.isfinite(total)
