"""GPU tier of the gradient planner (mjpc_hip::GradientPlanner through cplanner.GradientPlanner): the C++ planner against the numpy mirror
of the planner loop on HipBackend in closed loop on the particle, the reference's GradientPlannerTest.Particle, the skip path, a failed
derivative, and the testspeed harness with planner_kind 3."""
import numpy as np
import pytest

import gradient_planner_cases as gc
import gradient_planner_mirror as gm
from mujoco_mpc_amd import cplanner
from mujoco_mpc_amd.modelgen import particle
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu


def _hip_mirror(m, task, mocap, be, P, rep, N, fd_tol=1e-5):
    def plan_all(state, time, knot_times, cand, r, H):
        o = be.plan(state=state, mocap=mocap, time=time, knot_times=knot_times, knot_values=cand[0], interpolation=r, num_trajectory=len(cand), horizon=H,
                    sigma=(0.0, 0.0), candidate_knots=cand)
        a = be.fetch_all(len(cand), H, P)
        a["returns"] = o["returns"]
        return a

    def derivatives(x, u, t, r):
        return be.trajectory_gradient(x, u, t, r, mocap=mocap, eps=fd_tol, centered=False)
    return gm.GradientPlannerMirror(m, plan_all, derivatives, P, rep, N)


@pytest.mark.parametrize("rep", [1, 0])
def test_cpp_gradient_planner_matches_the_mirror_in_closed_loop_on_the_particle(rep):
    """six plan steps with the world stepped between them; per plan step: line-search steps and M' k bit-equal (the same device gradient
    goes through the same host arithmetic), returns at 1e-9 (the bar of test_gpu_sample_gradient.py's closed loop), the same winner, the
    policy bit-equal; zero and linear representation (there the engine's spline and GradientPolicy::Action are the same bits)"""
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    H, P, N = 16, 6, 12
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    world = HipBackend(m, task, max_samples=1, max_horizon=2)
    mir = _hip_mirror(m, task, mocap, be, P, rep, N)
    cpp = cplanner.GradientPlanner()
    cpp.Initialize(m, task, dict(gradient_spline_points=P, gradient_representation=rep, gradient_num_trajectory=N), max_samples=N, max_horizon=H)
    cpp.Reset(H)
    x = np.array([0.3, -0.2, 0.0, 0.0]); t = 0.0
    first = None
    for it in range(6):
        cpp.SetState(x, mocap, None, t); cpp.OptimizePolicy(H)
        mir.set_state(x, t); mir.optimize(H)
        v = cpp.values()
        assert not v["failed"] and not mir.failed
        assert np.array_equal(cpp.linesearch_steps(), np.array(mir.steps)), it
        assert np.array_equal(cpp.parameter_update(), mir.update), it
        r = cpp.returns(N)
        assert np.abs(r - mir.returns).max() <= 1e-9 * max(1.0, np.abs(mir.returns).max()), it
        assert v["winner"] == mir.winner and v["action_step"] == mir.action_step, it
        kt, kv = cpp.policy_knots()
        assert np.array_equal(kt, mir.times) and np.array_equal(kv, mir.parameters), it
        best = cpp.BestTrajectory()
        assert best.horizon == H and np.abs(best.states - mir.best["states"]).max() < 1e-9
        first = first if first is not None else best.total_return
        for _ in range(2):                                          # the world moves two steps under the new policy
            u = cpp.ActionFromPolicy(t)
            assert np.array_equal(u, mir.action(t))
            o = world.plan(state=x, mocap=mocap, time=t, knot_times=np.array([t]), knot_values=u[None, :], interpolation=0, num_trajectory=1, horizon=2,
                           sigma=(0.0, 0.0))
            x = o["states"][1].copy(); t = float(o["times"][1])
    assert best.total_return < first
    tm_ = cpp.timings()
    assert tm_["derivative_us"] > 0 and tm_["rollouts_us"] > 0
    for o in (be, world, cpp):
        o.close()


def test_reference_gradient_planner_particle():
    """GradientPlannerTest.Particle: 50 iterations, 26 steps of 0.1 s, 11 linear spline points, 32 candidates: the final position within
    1e-2 of the goal, the final velocity within 1e-1, all actions inside the ctrlrange"""
    c = gc.PARTICLE_TEST
    m, task, d = particle(timestep=c["timestep"])
    cpp = cplanner.GradientPlanner()
    cpp.Initialize(m, task, dict(gradient_spline_points=c["spline_points"], gradient_num_trajectory=c["num_trajectory"]), max_samples=c["num_trajectory"],
                   max_horizon=c["steps"])
    cpp.Reset(c["steps"])
    cpp.SetState(d["state"], d["mocap"], None, 0.0)
    for _ in range(c["iterations"]):
        cpp.OptimizePolicy(c["steps"])
    best = cpp.BestTrajectory()
    xf = best.states[c["steps"] - 1]
    print("final state", xf, "goal", d["mocap"][:2], "return", best.total_return)
    assert abs(xf[0] - d["mocap"][0]) < 1e-2 and abs(xf[1] - d["mocap"][1]) < 1e-2
    assert abs(xf[2]) < 1e-1 and abs(xf[3]) < 1e-1
    rng = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2)
    a = best.actions[:c["steps"] - 1]
    assert (a <= rng[:, 1]).all() and (a >= rng[:, 0]).all()
    cpp.close()


def test_skip_path_and_a_failed_derivative():
    """derivative_skip > 0 runs the composed path (ModelDerivatives, CostDerivatives, host Gradient) and improves the return; a NaN state
    fails the derivatives: OptimizePolicy stops like gd_status != 0 and leaves the policy as it was"""
    m, task, d = particle(timestep=0.1)
    H = 16
    fused = cplanner.GradientPlanner(); skip = cplanner.GradientPlanner()
    fused.Initialize(m, task, dict(gradient_spline_points=6, gradient_num_trajectory=8), max_samples=8, max_horizon=H)
    skip.Initialize(m, task, dict(gradient_spline_points=6, gradient_num_trajectory=8, derivative_skip=2), max_samples=8, max_horizon=H)
    x = np.array([0.3, -0.2, 0.0, 0.0])
    for p in (fused, skip):
        p.Reset(H); p.SetState(x, d["mocap"], None, 0.0); p.OptimizePolicy(H)
        v = p.values()
        assert not v["failed"] and v["improvement"] > 0 and v["winner"] < 7
    assert np.abs(fused.parameter_update() - skip.parameter_update()).max() < 0.2 * np.abs(fused.parameter_update()).max()   # interpolated blocks: close, not equal
    kt, kv = fused.policy_knots()
    bad = x.copy(); bad[0] = np.nan
    fused.SetState(bad, d["mocap"], None, 0.0); fused.OptimizePolicy(H)
    assert fused.values()["failed"]
    kt2, kv2 = fused.policy_knots()
    assert np.array_equal(kt, kt2) and np.array_equal(kv, kv2)
    fused.close(); skip.close()


def test_closed_loop_harness_drives_the_gradient_planner_like_the_manual_loop():
    """cplanner.testspeed with planner_kind 3 against the loop of testspeed.cc:97-116 written out by hand over a second planner: the cost
    per step is bit-equal"""
    m, task, d = particle(timestep=0.1)
    H, N, steps = 11, 8, 30
    num = dict(gradient_spline_points=5, gradient_num_trajectory=N)

    def make():
        p = cplanner.GradientPlanner()
        p.Initialize(m, task, num, max_samples=N, max_horizon=H)
        p.Reset(H)
        return p
    x0 = np.array([0.4, -0.3, 0.0, 0.0])
    a = make()
    res = cplanner.testspeed(a, x0, d["mocap"], horizon=H, steps_per_planning_iteration=2, total_time=steps * m["timestep"])
    assert res["plan_steps"] == steps // 2 and not res["failure"] and len(res["cost_per_step"]) == steps
    b = make()
    world = HipBackend(m, task, max_samples=1, max_horizon=2)
    x = x0.copy(); t = 0.0; costs = []
    for i in range(steps):
        u = b.ActionFromPolicy(t)
        out = world.plan(state=x, mocap=d["mocap"], time=t, knot_times=np.array([t]), knot_values=u[None, :], interpolation=0,
                         num_trajectory=1, horizon=2, sigma=(0.0, 0.0))
        costs.append(out["costs"][0])
        if i % 2 == 0:
            b.SetState(x, d["mocap"], None, t); b.OptimizePolicy(H)
        x = out["states"][1].copy(); t = out["times"][1]
    assert np.array_equal(res["cost_per_step"], np.array(costs))
    assert np.array_equal(res["state"], x)
    assert res["cost_per_step"][-5:].mean() < res["cost_per_step"][:5].mean()
    world.close(); a.close(); b.close()
