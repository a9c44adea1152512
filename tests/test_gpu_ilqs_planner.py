"""GPU tier of the iLQS planner (mjpc_hip::iLQSPlanner through cplanner.iLQSPlanner): the C++ planner against the numpy mirror
(ilqs_planner_mirror over host_mirror.SamplingPlanner and ilqg_planner_mirror on HipBackend) in closed loop on the particle, its branches
forced one by one, the refusals, and the testspeed harness with planner kind 5."""
import numpy as np
import pytest

import feedback_cases as fc
import host_mirror as hm
import ilqg_planner_mirror as im
import ilqs_planner_mirror as sm
from mujoco_mpc_amd import cplanner
from mujoco_mpc_amd.modelgen import particle, quadruped
from mujoco_mpc_amd.planner import HipBackend

pytestmark = pytest.mark.gpu

H, NS, NI, P = 16, 16, 8, 4
X0 = np.array([0.3, -0.2, 0.0, 0.0])
# the seed of the injected noise rows per sampling representation: with it all three branches occur within the eight plan steps, with and
# without a sliding plan
NOISE_SEED = {1: 0, 2: 0}


def _numerics(rep, exploration, spline_points=P, sliding_plan=1):
    return dict(sampling_trajectories=NS, sampling_representation=rep, sampling_spline_points=spline_points, sampling_exploration=exploration,
                sampling_sliding_plan=sliding_plan, ilqg_num_rollouts=NI, ilqg_representation=1)


def _cpp(m, task, rep, exploration, horizon=H, settings=None, **kw):
    cpp = cplanner.iLQSPlanner()
    cpp.Initialize(m, task, _numerics(rep, exploration, **kw), settings=settings, max_samples=NS, max_horizon=horizon)
    cpp.Reset(horizon)
    return cpp


def _noise(rng):
    return rng.standard_normal((NS, P, 2)), np.zeros(NS, np.int32)


def _mirror(m, task, mocap, rep, be_s, be_i, sliding):
    ms = hm.SamplingPlanner(be_s)
    ms.Initialize(m, task, _numerics(rep, 0.0, sliding_plan=sliding)); ms.Allocate(); ms.Reset(H)

    def rollouts(state, time, Hh, pol, mode, r, alpha, scale, improvement):
        o = be_i.plan_feedback(state, time, Hh, pol["times"], pol["states"], pol["actions"], pol["K"], alpha, scale,
                               action_improvement=pol["k"] if improvement else None, mode=mode, representation=r, mocap=mocap)
        return dict(returns=o["returns"], failure=o["failure"], rows=lambda i: be_i.candidate(i, Hh, 0))

    def backward(x, u, t, res, reg, rate):
        return be_i.trajectory_ilqg(x, u, t, res, mocap=mocap, eps=1e-6, centered=False, regularization=reg, regularization_rate=rate)
    return sm.ILQSPlannerMirror(m, ms, im.ILQGPlannerMirror(m, rollouts, backward, H, NI, 1), P)


def _close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(1.0, np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("sliding", [1, 0], ids=["sliding", "resampled"])
@pytest.mark.parametrize("rep", [1, 2], ids=["linear", "cubic"])
def test_cpp_ilqs_planner_matches_the_mirror_in_closed_loop_on_the_particle(rep, sliding):
    """eight plan steps, the world stepped twice between them.  Steps 0 and 1 run with noise_exploration = 0 (no candidate can beat member 0:
    the iLQG iteration is forced, and step 1 converts iLQG's nominal), from step 2 on with 0.2 and injected noise rows.  With a sliding plan
    the fitted knots are what sampling rolls out; without one sampling resamples its own last winner (header of iLQSPlanner)."""
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    be_s = HipBackend(m, task, max_samples=NS, max_horizon=H); be_i = HipBackend(m, task, max_samples=NI, max_horizon=H)
    world = HipBackend(m, task, max_samples=1, max_horizon=2)
    mir = _mirror(m, task, mocap, rep, be_s, be_i, sliding)
    cpp = _cpp(m, task, rep, 0.0, sliding_plan=sliding)
    rng = np.random.default_rng(NOISE_SEED[rep])
    x = X0.copy(); t = 0.0
    seen = dict(converted=0, seeded=0, early=0)
    for it in range(8):
        sigma = 0.0 if it < 2 else 0.2
        eps, sel = _noise(rng)
        cpp.set_noise_exploration(sigma); cpp.sampling.set_noise(eps, sel)
        mir.sampling.noise_exploration = [sigma, 0.0]; mir.sampling.injected_noise = (eps, sel)
        cpp.SetState(x, mocap, None, t); cpp.OptimizePolicy(H)
        mir.set_state(x, mocap, t); mir.optimize(H)
        v = cpp.values()
        print("step", it, v, "sampling winner", cpp.sampling.winner, "ilqg", cpp.ilqg.values()["winner"], cpp.ilqg.values()["action_step"])
        assert (v["active_policy"], v["previous_active_policy"]) == (mir.active, mir.previous_active), it
        assert (v["converted"], v["returned_early"], v["iterated"], v["adopted"]) == (mir.converted, mir.returned_early, mir.iterated, mir.adopted), it
        assert cpp.sampling.winner == mir.sampling.winner, it
        assert _close(cpp.sampling.returns(NS), mir.sampling.returns), it
        seen["converted"] += v["converted"]; seen["early"] += v["returned_early"]
        seen["seeded"] += v["iterated"] and v["previous_active_policy"] == sm.kSampling
        if v["converted"]:
            kt, kv = cpp.fitted_knots()
            assert np.array_equal(kt, mir.fitted[0]) and np.array_equal(kv, mir.fitted[1]), it
        if v["iterated"]:
            assert _close(cpp.ilqg.returns(NI), mir.ilqg.returns), it
        if v["adopted"]:
            w = cpp.ilqg.values()
            assert w["winner"] == mir.ilqg.winner and w["action_step"] == mir.ilqg.action_step, it
            p = cpp.ilqg.get_policy(0)
            assert np.array_equal(p["actions"], mir.ilqg.policy["actions"][:H]), it
            assert np.array_equal(p["feedback_gain"], mir.ilqg.policy["K"][:H]) and np.array_equal(p["action_improvement"], mir.ilqg.policy["k"][:H]), it
        for tq in (t, t + 0.05, t + 0.7):
            for st in (None, x + 0.01):
                for prev in (False, True):
                    a = cpp.ActionFromPolicy(tq, use_previous=prev, state=st)
                    with fc.summation_rule():
                        assert np.array_equal(a, mir.action(tq, st, use_previous=prev, H=H)), (it, tq, prev)
        # BestTrajectory is the active member's
        best = cpp.BestTrajectory()
        member = cpp.sampling.BestTrajectory() if v["active_policy"] == sm.kSampling else cpp.ilqg.BestTrajectory()
        assert best.horizon == H and np.array_equal(best.states, member.states) and best.total_return == member.total_return, it
        ms, mr = mir.best()
        assert np.abs(best.states - ms[:H]).max() < 1e-9 and _close(best.total_return, mr), it
        for _ in range(2):
            u = cpp.ActionFromPolicy(t, state=x)
            o = world.step_batch(x[None], u[None], np.array([t]), mocap=mocap)
            x = o["next_states"][0]; t += 0.1
    print("branches seen:", seen)
    assert seen["converted"] >= 1, "no conversion from iLQG"
    assert seen["seeded"] >= 1, "no iteration seeded from sampling.trajectory[0]"
    assert seen["early"] >= 1, "sampling never returned early"
    be_s.close(); be_i.close(); world.close()


def _particle_planner(exploration, settings=None, rep=1, **kw):
    m, task, d = particle(timestep=0.1)
    mocap = np.asarray(d["mocap"], float)
    cpp = _cpp(m, task, rep, exploration, settings=settings, **kw)
    cpp.SetState(X0, mocap, None, 0.0)
    return cpp, mocap


def test_zero_noise_seeds_the_iteration_from_sampling_member_0():
    cpp, _ = _particle_planner(0.0)
    cpp.OptimizePolicy(H)
    v = cpp.values()
    assert v["previous_active_policy"] == sm.kSampling and v["iterated"] and not v["converted"] and not v["returned_early"]
    assert cpp.sampling.winner == 0
    m0 = cpp.sampling_member(0, H)
    a0 = m0["actions"].copy(); a0[H - 1] = a0[H - 2]
    c = cpp.ilqg.get_policy(2)
    w = cpp.ilqg.values()
    assert v["adopted"] and w["winner"] >= 0
    if w["winner"] == 0:            # the reference has overwritten slot 0 with the winning rollout
        best = cpp.ilqg.BestTrajectory()
        assert np.array_equal(c["states"], best.states) and np.array_equal(c["actions"], best.actions)
    else:                           # the nominal's states, its actions moved along the improvement by the winning step
        assert np.array_equal(c["states"], m0["states"]) and np.array_equal(c["times"], m0["times"])
        assert np.array_equal(c["actions"], a0 + c["action_improvement"] * w["action_step"])
    # sampling's best trajectory is still its winner's
    sb = cpp.sampling.BestTrajectory()
    assert np.array_equal(sb.states, m0["states"]) and sb.total_return == m0["total_return"] == cpp.sampling.returns(NS)[0]
    assert v["active_policy"] == (sm.kiLQG if cpp.ilqg.BestTrajectory().total_return < sb.total_return else sm.kSampling)


def test_an_iteration_that_adopts_nothing_leaves_the_active_policy():
    cpp, _ = _particle_planner(0.0, settings=dict(max_regularization_iterations=0))
    cpp.OptimizePolicy(H)
    v = cpp.values()
    assert v["iterated"] and not v["adopted"] and cpp.ilqg.values()["backward_pass_failed"]
    assert v["active_policy"] == sm.kSampling and v["previous_active_policy"] == sm.kSampling
    # the nominal handed over is sampling's member 0, bit for bit, the last action row repeating the one before
    m0 = cpp.sampling_member(0, H)
    c = cpp.ilqg.get_policy(2)
    assert np.array_equal(c["states"], m0["states"]) and np.array_equal(c["times"], m0["times"])
    assert np.array_equal(c["actions"][:H - 1], m0["actions"][:H - 1]) and np.array_equal(c["actions"][H - 1], m0["actions"][H - 2])
    assert np.array_equal(cpp.sampling.BestTrajectory().states, cpp.sampling_member(cpp.sampling.winner, H)["states"])
    assert np.array_equal(cpp.BestTrajectory().states, cpp.sampling.BestTrajectory().states)


def test_an_early_return_leaves_ilqg_untouched():
    cpp, _ = _particle_planner(0.2)
    eps, sel = _noise(np.random.default_rng(5))
    cpp.sampling.set_noise(eps, sel)
    before = cpp.ilqg.get_policy(0)
    cpp.OptimizePolicy(H)
    v = cpp.values()
    r = cpp.sampling.returns(NS)
    print("sampling winner", cpp.sampling.winner, "returns", r[cpp.sampling.winner], "against member 0", r[0])
    assert v["returned_early"] and not v["iterated"] and v["active_policy"] == sm.kSampling
    assert cpp.sampling.winner > 0 and r[cpp.sampling.winner] < r[0]
    after = cpp.ilqg.get_policy(0)
    for k in ("times", "states", "actions", "feedback_gain", "action_improvement"):
        assert np.array_equal(before[k], after[k]), k
    tm = cpp.ilqg.timings()
    assert tm["derivative_us"] == 0 and tm["rollouts_us"] == 0 and tm["policy_update_us"] == 0 and tm["nominal_us"] == 0
    # fetching another member leaves sampling's best trajectory its winner's
    w = cpp.sampling_member(cpp.sampling.winner, H)
    cpp.sampling_member(0, H)
    sb = cpp.sampling.BestTrajectory()
    assert np.array_equal(sb.states, w["states"]) and sb.total_return == r[cpp.sampling.winner]
    assert np.array_equal(cpp.BestTrajectory().states, sb.states)


@pytest.mark.parametrize("kw", [dict(rep=0), dict(spline_points=1), dict(spline_points=26)], ids=["zero-order", "P=1", "P=26"])
def test_initialize_refuses_what_the_fit_cannot_do(kw):
    m, task, d = particle(timestep=0.1)
    kw = dict(dict(rep=1), **kw)
    with pytest.raises(cplanner.PlannerError):
        _cpp(m, task, kw.pop("rep"), 0.0, **kw)


def test_a_singular_fit_is_refused_and_leaves_the_sampling_plan():
    """linear with P = H = 8: a knot at every step, the last one behind the last action"""
    Hs = 8
    cpp, mocap = _particle_planner(0.0, horizon=Hs, spline_points=Hs)
    cpp.OptimizePolicy(Hs)              # zero noise: the iteration runs and iLQG takes over
    assert cpp.values()["active_policy"] == sm.kiLQG
    kt, kv = cpp.sampling.policy_knots()
    cpp.SetState(X0, mocap, None, 0.1)
    with pytest.raises(cplanner.PlannerError, match="singular"):
        cpp.OptimizePolicy(Hs)
    kt2, kv2 = cpp.sampling.policy_knots()
    assert np.array_equal(kt, kt2) and np.array_equal(kv, kv2)
    assert not cpp.values()["converted"] and cpp.values()["active_policy"] == sm.kiLQG


def test_testspeed_kind_5_runs_the_a1():
    m, task, d = quadruped()
    Hq, N = 12, 8
    cpp = cplanner.iLQSPlanner()
    cpp.Initialize(m, task, dict(sampling_trajectories=N, sampling_representation=2, sampling_spline_points=3, sampling_exploration=0.04, ilqg_num_rollouts=N),
                   max_samples=N, max_horizon=Hq)
    cpp.Reset(Hq)
    o = cplanner.testspeed(cpp, d["state"], d["mocap"], horizon=Hq, steps_per_planning_iteration=4, total_time=float(m["timestep"]) * 12)
    print("testspeed kind 5: total cost", o["total_cost"], "plan steps", o["plan_steps"], "failure", o["failure"], cpp.values())
    assert not o["failure"] and o["plan_steps"] >= 3 and np.isfinite(o["total_cost"])
