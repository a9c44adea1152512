"""GPU tier of the Sample-Gradient planner: the mixed plan step (mjpc_hip_plan_mixed) against plain plans and the oracle, the
device gradient sum (mjpc_hip_sample_gradient) against the sequential numpy loop, the C++ planner against the Python mirror on the
oracle in closed loop (particle, OP3 Stand), and the testspeed harness driving the new planner."""
import numpy as np
import pytest

import oracle_lib as ol
import sample_gradient_mirror as sgm
from mujoco_mpc_amd.modelgen import humanoid_track, op3, particle, quadruped
from mujoco_mpc_amd.planner import HipBackend
from oracle_backend import OracleBackend
from spill_common import with_capacity

pytestmark = pytest.mark.gpu

ROWS = ("states", "actions", "times", "residual", "costs", "trace", "knots")


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


# ----------------------------------------------------------------------------- (a) the mixed plan step
def _mixed_case(m, task, d, N, H, P, fe, tol, expect):
    nu = m["nu"]
    rng = np.random.default_rng(12)
    kt = np.linspace(0, (H - 1) * m["timestep"], P); kv = rng.uniform(-0.1, 0.1, (P, nu))
    std = rng.uniform(0.02, 0.12, P * nu)
    explicit = rng.uniform(-0.2, 0.2, (N, P, nu))
    mocap = d["mocap"] if len(d["mocap"]) else None
    seed, stream = 21, 3
    common = dict(state=d["state"], mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=2, num_trajectory=N, horizon=H,
                  sigma=(0.0, 0.0), seed=seed, stream=stream)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    expect(be)
    noisy = be.plan(noise_std=std, nominal_index=0, **common); noisy_all = be.fetch_all(N, H, P)
    given = be.plan(candidate_knots=explicit, **common); given_all = be.fetch_all(N, H, P)
    mixed = be.plan_mixed(fe, noise_std=std, nominal_index=0, candidate_knots=explicit, **common); mixed_all = be.fetch_all(N, H, P)
    used_dense = be.dense_tier()[1]
    # rows below first_explicit: a plain plan with the same noise_std and seed, bit for bit; rows from it on: the explicit plan
    assert np.array_equal(mixed["returns"][:fe], noisy["returns"][:fe]) and np.array_equal(mixed["returns"][fe:], given["returns"][fe:])
    assert np.array_equal(mixed["failure"][:fe], noisy["failure"][:fe]) and np.array_equal(mixed["failure"][fe:], given["failure"][fe:])
    for k in ROWS:
        assert np.array_equal(mixed_all[k][:fe], noisy_all[k][:fe]), k
        assert np.array_equal(mixed_all[k][fe:], given_all[k][fe:]), k
    assert np.array_equal(mixed_all["knots"][0], kv) and np.array_equal(mixed_all["knots"][fe:], explicit[fe:])
    assert mixed["winner"] == int(np.argmin(mixed["returns"])) and np.array_equal(mixed["states"], mixed_all["states"][mixed["winner"]])
    # a shard of the same batch across the boundary: candidate_offset / num_local work as for any plan
    off, nl = fe - 5, 11
    shard = be.plan_mixed(fe, noise_std=std, nominal_index=0, candidate_knots=explicit, candidate_offset=off, num_local=nl, **common)
    shard_all = be.fetch_all(nl, H, P)
    assert np.array_equal(shard["returns"], mixed["returns"][off:off + nl]) and np.array_equal(shard_all["knots"], mixed_all["knots"][off:off + nl])
    # every row against the oracle at the parity suite's bars.  The device's Box-Muller may differ from glibc's in the last ulp
    # (test_device_philox_matches_oracle_noise), so this plan takes the oracle's evaluation of the same Philox stream as injected noise
    eps, _ = ol.noise(seed, stream, 0, N, P, nu)
    seeded_knots = mixed_all["knots"]
    mixed = be.plan_mixed(fe, noise_std=std, nominal_index=0, candidate_knots=explicit, noise_eps=eps, **common); mixed_all = be.fetch_all(N, H, P)
    assert np.abs(mixed_all["knots"] - seeded_knots).max() < 1e-14
    be.close()
    o = ol.Oracle(m, task)
    ra = o.plan(d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.0, 0.0), noise_eps=eps, noise_std=std, nominal_index=0, num_local=fe, nthreads=8)
    rb = o.plan(d["state"], mocap, 0.0, kt, kv, 2, N, H, sigma=(0.0, 0.0), candidate_knots=explicit, candidate_offset=fe, num_local=N - fe, nthreads=8)
    ref = {k: np.concatenate([ra[k], rb[k]]) for k in ROWS + ("returns", "failure")}
    assert np.array_equal(mixed["failure"], ref["failure"])
    assert np.array_equal(mixed_all["knots"], ref["knots"])
    ok = mixed["failure"] == 0
    assert ok.any() and np.array_equal(mixed_all["times"][ok], ref["times"][ok])
    assert _rel(mixed_all["actions"][ok], ref["actions"][ok]) < 1e-14
    for k in ("states", "residual", "costs", "trace"):
        assert _rel(mixed_all[k][ok], ref[k][ok]) < tol, k
    assert _rel(mixed["returns"], ref["returns"]) < tol
    assert mixed["winner"] == int(np.argmin(ref["returns"]))
    return used_dense


def test_mixed_plan_rows_are_the_plain_plans_rows_and_match_the_oracle_on_the_quadruped():
    m, task, d = quadruped()
    used = _mixed_case(m, task, d, 64, 30, 3, 48, 1e-5, lambda be: None)
    assert not used


def test_mixed_plan_on_the_forced_dense_tier(debug_knobs):
    m, task, d = quadruped()
    debug_knobs("tier", "B")

    def expect(be):
        assert be.dense_tier()[0] > 0
    assert _mixed_case(m, task, d, 64, 30, 3, 48, 1e-5, expect)


def test_mixed_plan_on_a_spill_flavour_model():
    m, task, d = with_capacity(humanoid_track(), 64, 192)

    def expect(be):
        assert be.spill_bytes() > 0
    _mixed_case(m, task, d, 64, 30, 4, 48, 1e-5, expect)


# ----------------------------------------------------------------------------- (b) the gradient sum
def test_sample_gradient_is_the_sequential_loop_bit_for_bit_and_repeatable():
    """History filled by one mixed plan on the quadruped with injected normals (4096 x 36 x 12: the C2 shape, P * nu = 432), then
    sums over n = 31 and n = 4095 slots; the slot lists hold slot 0, explicit slots and a repeat."""
    m, task, d = quadruped()
    N, H, P, nu, fe = 4096, 2, 36, 12, 3584
    PN = P * nu
    rng = np.random.default_rng(8)
    eps = rng.standard_normal((N, P, nu))
    kt = np.linspace(0, 0.35, P); kv = np.zeros((P, nu))
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    with pytest.raises(RuntimeError, match="no mixed plan"):
        be.sample_gradient([1], [1.0])
    be.plan_mixed(fe, state=d["state"], mocap=d["mocap"], time=0.0, knot_times=kt, knot_values=kv, interpolation=0, num_trajectory=N, horizon=H,
                  sigma=(0.0, 0.0), noise_eps=eps, noise_std=np.full(PN, 0.01), nominal_index=0, candidate_knots=np.zeros((N, P, nu)))
    hist = np.zeros((N, PN)); hist[1:fe] = eps[1:fe].reshape(fe - 1, PN)
    for n in (31, 4095):
        slot = rng.integers(1, fe, n).astype(np.int32)
        slot[0] = 0; slot[1] = fe + 7; slot[2] = N - 1; slot[-1] = slot[5]
        scale = rng.standard_normal(n) / n
        g1 = be.sample_gradient(slot, scale)
        g2 = be.sample_gradient(slot, scale)
        want = sgm.sequential_gradient(hist, slot, scale, PN)
        assert g1.shape == (PN,) and np.array_equal(g1, g2)
        assert np.array_equal(g1, want), np.abs(g1 - want).max()
    # out-of-range arguments are refused on the host, before any launch
    for bad_slot, bad_scale, what in (([0, N], [1.0, 1.0], "slot"), ([-1], [1.0], "slot"), ([], [], "n out of range")):
        with pytest.raises(RuntimeError, match=what):
            be.sample_gradient(np.array(bad_slot, np.int32), np.array(bad_scale, float))
    # reset zeroes the history; a smaller P afterwards only writes the head of a slot
    be.noise_history_reset()
    assert not be.sample_gradient(np.arange(1, 40, dtype=np.int32), np.ones(39)).any()
    be.close()


def test_history_keeps_slot_zero_explicit_slots_and_a_stale_tail_on_the_device():
    m, task, d = particle(timestep=0.1)
    N, H, nu = 10, 3, 2
    rng = np.random.default_rng(4)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)

    def plan(P, fe):
        eps = rng.standard_normal((N, P, nu))
        be.plan_mixed(fe, state=d["state"], mocap=d["mocap"], time=0.0, knot_times=np.linspace(0, 0.2, P), knot_values=np.zeros((P, nu)),
                      interpolation=0, num_trajectory=N, horizon=H, sigma=(0.0, 0.0), noise_eps=eps, noise_std=np.full(P * nu, 0.1),
                      nominal_index=0, candidate_knots=np.zeros((N, P, nu)))
        return eps

    def slot_rows(P):      # one-hot sums read the slots back: gradient = history[s] * 1.0
        return np.array([be.sample_gradient(np.array([s], np.int32), np.ones(1)) for s in range(N)])
    e1 = plan(6, 8)
    h = slot_rows(6)
    assert not h[0].any() and not h[8:].any() and np.array_equal(h[1:8], e1[1:8].reshape(7, 12))
    e2 = plan(4, 6)
    plan_tail = slot_rows(4)
    assert np.array_equal(plan_tail[1:6], e2[1:6].reshape(5, 8)) and np.array_equal(plan_tail[6:8], e1[6:8].reshape(2, 12)[:, :8])
    e3 = plan(6, 6)                                                 # back to 6 points: rows 6, 7 are explicit now and keep plan 1's noise
    h = slot_rows(6)
    assert np.array_equal(h[1:6], e3[1:6].reshape(5, 12)) and np.array_equal(h[6:8], e1[6:8].reshape(2, 12)) and not h[0].any() and not h[8:].any()
    e4 = plan(4, 3); h4 = slot_rows(4)
    plan(6, 1); h = slot_rows(6)                                    # no noisy row at all: nothing is written, the tail of plan 3 is still there
    assert np.array_equal(h[1:3, :8], e4[1:3].reshape(2, 8)) and np.array_equal(h[1:3, 8:], e3[1:3].reshape(2, 12)[:, 8:]) and h4.shape == (N, 8)
    be.close()


# ----------------------------------------------------------------------------- (c), (d) the C++ planner against the mirror
def _closed_loop(m, task, d, num, H, iters, seed, state, mocap, backend, action0, ret_tol):
    from mujoco_mpc_amd import cplanner
    N, ng, P = num["sampling_trajectories"], num["sample_gradient_trajectories"], num["sampling_spline_points"]
    nu = m["nu"]
    cpp = cplanner.SampleGradientPlanner()
    cpp.Initialize(m, task, num, max_samples=N, max_horizon=H)
    cpp.Reset(H, action0); cpp.set_seed(seed, 0)
    ref = sgm.SampleGradientMirror(backend, m, task, num)
    ref.Reset(H, action0); ref.seed = seed; ref.plan_iter = 0
    t = 0.0
    types = []
    for it in range(iters):
        # both sides draw Philox(seed, stream = iteration); the C++ planner gets the oracle's evaluation of it injected, because the
        # device's Box-Muller may differ from glibc's in the last ulp and the comparison below is bit for bit
        eps, _ = ol.noise(seed, it, 0, N, P, nu)
        cpp.set_noise(eps)
        cpp.SetState(state, mocap, None, t); ref.SetState(state, mocap, None, t)
        cpp.OptimizePolicy(H); ref.OptimizePolicy(H)
        # precondition, on the oracle's numbers alone: the ranks are decided by gaps far above the GPU-versus-oracle return error
        gap = ref.min_rank_gap()
        print(f"iteration {it}: min rank gap {gap:.2e} winner {ref.winner} type {ref.winner_type} return error {_rel(cpp.returns(N), ref.returns):.2e}")
        assert gap >= 1e-6, (it, gap)
        assert not ref.failure.any()
        assert _rel(cpp.returns(N), ref.returns) < ret_tol
        assert np.array_equal(cpp.trajectory_order(N), ref.order[:N])
        assert cpp.winner == ref.winner and cpp.winner_type_ == ref.winner_type
        assert cpp.num_gradient_ == ng
        assert np.array_equal(cpp.gradient(), ref.gradient[:P * nu])
        kt, kv = cpp.policy_knots()
        rt, rv = ref.policy.plan.arrays()
        assert np.array_equal(kt, rt) and np.array_equal(kv, rv)
        for i in range(N):
            ct, cv = cpp.candidate_policy(i)
            mt, mv = ref.candidate[i].plan.arrays()
            assert np.array_equal(ct, mt) and np.array_equal(cv, mv), i
        assert np.array_equal(cpp.return_weight(), ref.return_weight) and np.array_equal(cpp.step_size(), ref.step_size)
        assert abs(cpp.improvement - ref.improvement) <= ret_tol * abs(ref.returns).max()
        best = cpp.BestTrajectory()
        assert best.horizon == H and _rel(best.states, ref.winner_states) < 1e-5 and best.total_return == cpp.returns(N)[cpp.winner]
        types.append(ref.winner_type)
        state = best.states[1].copy(); t += m["timestep"]
    cpp.close()
    return state, types


@pytest.mark.parametrize("interp", [0, 2])
def test_cpp_sample_gradient_planner_matches_the_mirror_in_closed_loop_on_the_particle(interp):
    """mjpc_hip::SampleGradientPlanner (C++; batch and gradient sum on the HIP engine) against the Python mirror on the CPU oracle,
    same Philox seed (evaluated by the oracle and injected into the C++ planner, so that both see the same bits), 30 plan iterations in closed loop: order, winner, winner type equal; gradient, policy knots, every candidate
    policy, weights and step sizes bit-equal; returns at 1e-9; the particle ends within 0.15 of the goal.
    Precondition, asserted at every iteration on the oracle's returns: adjacent sorted returns of non-failed candidates differ by
    at least 1e-6 relative (the bit-equality rests on equal ranks; the return bar is 1e-9).  Candidates whose knots are bit-identical
    are one policy with one return and are counted once: after Reset the reference's gradient candidates are all the empty plan, so
    the first plan step holds six identical all-zero policies (and the nominal is a seventh), whatever the seed.
    Seed 17: the mirror alone, in closed loop on its own states, has a smallest gap of 3.5e-5 (zero-order hold) / 4.8e-5 (cubic)
    over the 30 iterations and ends 0.014 / 0.047 from the goal (checked on the CPU; seeds 1..39 gave 2.7e-8 .. 9.0e-5)."""
    m, task, d = particle(timestep=0.1)
    H, N = 20, 24
    num = dict(sampling_spline_points=5, sampling_exploration=0.2, sampling_trajectories=N, sample_gradient_trajectories=6,
               sampling_representation=interp)
    state, types = _closed_loop(m, task, d, num, H, 30, 17, np.array([0.3, -0.2, 0.0, 0.0]), d["mocap"], OracleBackend(m, task), None, 1e-9)
    assert np.abs(state[:2] - d["mocap"][:2]).sum() < 0.15
    assert sgm.kGradient in types and sgm.kPerturb in types           # both kinds of candidate did win along the way


def test_cpp_sample_gradient_planner_matches_the_mirror_on_op3_stand():
    """OP3 Stand with its task.xml numbers (32 trajectories of which 8 gradient, 3 cubic spline points, exploration 0.1, horizon 24),
    modelgen's model, five plan iterations, same assertions and precondition as the particle test.  The oracle writes no residual
    rows for this task, so the mirror's backend takes the oracle's states and actions through tests/task_ref.py
    (sample_gradient_mirror.ResidualRefBackend).  Seed 9: the mirror alone has gaps 3.0e-3, 5.0e-4, 1.6e-4, 1.5e-3, 2.4e-4 and its
    winners are perturbed, gradient, nominal, gradient, nominal (checked on the CPU; seeds 1..12 gave smallest gaps 1.5e-6 .. 3.2e-4)."""
    m, task, d = op3()
    num = dict(sampling_spline_points=3, sampling_exploration=0.1, sampling_trajectories=32, sample_gradient_trajectories=8,
               sampling_representation=d["interp"])
    _closed_loop(m, task, d, num, d["horizon"], 5, 9, d["state"].copy(), None, sgm.ResidualRefBackend(m, task), d["ctrl0"], 1e-9)


# ----------------------------------------------------------------------------- (e) the testspeed harness
def test_closed_loop_harness_drives_the_sample_gradient_planner_like_the_manual_loop():
    """cplanner.testspeed with the new planner (planner_kind 2) against the loop of testspeed.cc:97-116 written out by hand over a
    second planner instance with the same seed: the cost per step is bit-equal, as for the sampling planner."""
    from mujoco_mpc_amd import cplanner
    m, task, d = particle(timestep=0.1)
    H, N, steps = 11, 16, 40
    num = dict(sampling_spline_points=6, sampling_exploration=0.2, sampling_trajectories=N, sample_gradient_trajectories=4, sampling_representation=2)

    def make():
        p = cplanner.SampleGradientPlanner()
        p.Initialize(m, task, num, max_samples=N, max_horizon=H)
        p.Reset(H); p.set_seed(7, 0)
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
    assert np.array_equal(a.gradient(), b.gradient()) and a.gradient().any()
    assert res["cost_per_step"][-10:].mean() < 0.3 * res["cost_per_step"][:5].mean()
    world.close(); a.close(); b.close()
