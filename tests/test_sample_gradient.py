"""Sample-Gradient planner, the tier that runs without a GPU: the host closed forms of the C++ planner against the mirror
(tests/sample_gradient_mirror.py), the mirror's own behaviour on the oracle (the quirks of planners/sample_gradient/planner.cc it
must keep), the device functions of csrc/gradient.h in the 1-lane emulation, and the new C ABI entry points as far as they go
without a device."""
import ctypes
import math

import numpy as np
import pytest

import emu_gradient_lib as eg
import emu_lib
import oracle_lib as ol
import sample_gradient_mirror as sgm
from mujoco_mpc_amd import capi, cplanner
from mujoco_mpc_amd.modelgen import particle
from oracle_backend import OracleBackend


# ----------------------------------------------------------------------------- host closed forms
@pytest.mark.parametrize("n_noisy", [2, 18, 24, 127])
def test_return_weights_sum_to_zero_and_match_the_cpp_closed_form(n_noisy):
    rng = np.random.default_rng(n_noisy)
    for order in (np.arange(n_noisy), rng.permutation(n_noisy), rng.permutation(n_noisy + 9)[:n_noisy]):      # the last one names "gradient slots"
        w = sgm.return_weights(order, n_noisy)
        assert abs(w.sum()) < 1e-15 * n_noisy / 2 and abs(math.fsum(w)) < 1e-15
        assert np.array_equal(w, cplanner.sample_gradient_return_weights(order))
    # index, not rank: candidate 0 always carries the largest weight, wherever it is ranked
    order = np.arange(n_noisy)[::-1].copy()
    w = sgm.return_weights(order, n_noisy)
    assert int(np.argmax(w)) == n_noisy - 1 and w[0] == w.min()


@pytest.mark.parametrize("steps", [1, 2, 6, 8, 512])
def test_step_sizes_run_from_the_minimum_to_the_maximum(steps):
    s = sgm.log_scale(2.0, 1.0e-3, steps)
    assert np.array_equal(s, cplanner.sample_gradient_step_sizes(steps))
    assert s[0] == 1.0e-3
    if steps > 1:
        top = math.exp(math.log(2.0))
        assert abs(s[-1] - top) <= math.ulp(top) and np.all(np.diff(s) > 0)


# ----------------------------------------------------------------------------- the mirror on the oracle
def _mirror(num, m, task, seed=5, max_samples=None, action0=None, H=12):
    r = sgm.SampleGradientMirror(OracleBackend(m, task), m, task, num, max_samples=max_samples)
    r.Reset(H, action0); r.seed = seed; r.plan_iter = 0
    return r


def test_without_gradient_candidates_the_policy_is_the_best_of_nominal_and_absolute_noise_candidates():
    m, task, d = particle(timestep=0.1)
    H, N, P, nu, sig = 12, 10, 4, 2, 0.25
    num = dict(sampling_spline_points=P, sampling_exploration=sig, sampling_trajectories=N, sample_gradient_trajectories=0, sampling_representation=1)
    ref = _mirror(num, m, task, seed=5, H=H)
    o = ol.Oracle(m, task)
    lo, hi = m["actuator_ctrlrange"].reshape(-1, 2).T
    from host_mirror import TimeSpline
    pol = TimeSpline(nu, 1)
    state = np.array([0.3, -0.2, 0.0, 0.0]); t = 0.0
    for it in range(6):
        ref.SetState(state, d["mocap"], None, t); ref.OptimizePolicy(H)
        # by hand: resample, perturb, roll out, take the best unless the nominal is at least as good
        shift = max((H - 1) * m["timestep"] / (P - 1), 1e-5)
        times = np.zeros(P); tt = t
        for k in range(P):
            times[k] = tt; tt += shift
        nominal = np.array([np.clip(pol.Sample(x), lo, hi) for x in times])
        eps, _ = ol.noise(5, it, 0, N, P, nu)
        knots = np.clip(nominal[None] + sig * eps, lo, hi); knots[0] = nominal
        out = o.plan(state, d["mocap"], t, times, np.zeros((P, nu)), 1, N, H, candidate_knots=knots)
        best = int(np.argmin(out["returns"]))
        win = best if out["returns"][best] < out["returns"][0] else 0
        assert ref.winner == win and ref.winner_type == (sgm.kPerturb if win else sgm.kNominal)
        assert np.array_equal(ref.returns, out["returns"])
        pol = TimeSpline(nu, 1)
        for k in range(P):
            pol.AddNode(times[k], knots[win, k])
        kt, kv = ref.policy.plan.arrays()
        assert np.array_equal(kt, times) and np.array_equal(kv, knots[win])
        assert not ref.gradient.any() and len(ref.return_weight) == 0          # GradientCandidates returns at once
        state = out["states"][win, 1].copy(); t += m["timestep"]


def test_weights_are_cached_and_a_gradient_slot_inside_the_first_noisy_ranks_contributes_its_zero_history():
    """Two quirks of planner.cc:419-459.  The weights are computed on the first plan (from the noisy candidates sorted among
    themselves) and never again.  From the second plan on the sum walks the first n_noisy entries of the FULL order: a gradient
    candidate ranked there is read from its own history slot, which no plan ever wrote."""
    m, task, d = particle(timestep=0.1)
    H, N, ng, P = 12, 12, 4, 3
    nn = N - ng
    num = dict(sampling_spline_points=P, sampling_exploration=0.2, sampling_trajectories=N, sample_gradient_trajectories=ng, sampling_representation=0)
    ref = _mirror(num, m, task, seed=3, H=H)
    state = np.array([0.4, -0.3, 0.0, 0.0]); t = 0.0
    ref.SetState(state, d["mocap"], None, t); ref.OptimizePolicy(H)
    w0 = ref.return_weight.copy()
    assert len(w0) == nn and sorted(ref.slots) == list(range(nn))             # first plan: the noisy candidates only
    assert np.array_equal(w0, sgm.return_weights(sgm.order_by_return(ref.returns[:nn]), nn))
    seen = False
    for it in range(1, 8):
        state = ref.winner_states[1].copy(); t += m["timestep"]
        ref.SetState(state, d["mocap"], None, t); ref.OptimizePolicy(H)
        assert np.array_equal(ref.return_weight, w0)                           # cached for good
        assert np.array_equal(ref.slots, ref.full_order[:nn])                  # the full sort's order, not a noisy-only one
        grad_slots = [s for s in ref.slots if s >= nn]
        if grad_slots:
            seen = True
            assert not ref.hist[grad_slots].any()                              # their slots are still zero ...
            keep = np.array([s < nn for s in ref.slots])
            g = sgm.sequential_gradient(ref.hist, ref.slots[keep], ref.scale[keep], P * 2)
            assert np.array_equal(ref.gradient[:P * 2], g)                     # ... so they add nothing (x + 0 * w = x)
        assert not ref.hist[0].any() and not ref.hist[nn:].any()
    assert seen                                                                # the case did come up in this run


# ----------------------------------------------------------------------------- device functions, 1-lane emulation
def test_emulated_assembly_matches_the_rollout_kernels_own_candidate_policies_bit_for_bit():
    m, task, d = particle(timestep=0.1)
    N, H, P, nu, fe = 9, 3, 5, 2, 6
    rng = np.random.default_rng(1)
    kt = np.linspace(0, 0.2, P); nominal = rng.uniform(-0.9, 0.9, (P, nu))
    std = rng.uniform(0.05, 0.6, P * nu)                                        # large enough that the clamp bites
    eps, _ = ol.noise(7, 2, 0, N, P, nu)
    plain = emu_lib.plan(m, task, d["state"], d["mocap"], 0.0, kt, nominal, 2, N, H, sigma=(0.0, 0.0), noise_eps=eps, noise_std=std, nominal_index=0)
    assert (np.abs(plain["knots"]) == 1.0).any()
    explicit = rng.uniform(-1, 1, (N, P, nu))
    for offset, nl in ((0, N), (2, 6), (7, 2)):
        cand = np.full((nl, P, nu), np.nan); hist = np.full((nl + 1, 36 * nu), 7.0)
        r0 = max(fe - offset, 0)
        cand[r0:] = explicit[offset + r0:offset + nl]                           # what the host copies in before the kernel runs
        eg.assemble(nominal.copy(), std, np.ascontiguousarray(eps[offset:offset + nl]), m["actuator_ctrlrange"].astype(float).ravel().copy(), cand, hist,
                    offset, 0, fe)
        for r in range(nl):
            gi = offset + r
            assert np.array_equal(cand[r], plain["knots"][gi] if gi < fe else explicit[gi]), (offset, r)
            want = np.full(36 * nu, 7.0)
            if 0 < gi < fe:
                want[:P * nu] = eps[gi].ravel()
            assert np.array_equal(hist[r], want)
        assert np.all(hist[nl] == 7.0)
        # the assembled table, fed back as explicit policies, rolls out to the same trajectories as the plain plan
        if offset == 0:
            again = emu_lib.plan(m, task, d["state"], d["mocap"], 0.0, kt, nominal, 2, N, H, sigma=(0.0, 0.0), candidate_knots=cand)
            assert np.array_equal(again["states"][:fe], plain["states"][:fe]) and np.array_equal(again["returns"][:fe], plain["returns"][:fe])


@pytest.mark.parametrize("n", [1, 7, 255, 4095])
def test_emulated_gradient_is_the_sequential_loop_bit_for_bit(n):
    PN, slots = 432, 4096
    rng = np.random.default_rng(n)
    hist = rng.standard_normal((slots, PN))
    hist[0] = 0.0; hist[4000:] = 0.0                                            # slot 0 and "explicit" slots
    slot = rng.integers(0, slots, n).astype(np.int32)
    slot[0] = 0
    if n > 2:
        slot[1] = 4090; slot[-1] = slot[2]                                      # an explicit slot; a repeated slot
    scale = rng.standard_normal(n) / n
    g = eg.gradient(hist, slot, scale, PN)
    assert np.array_equal(g, sgm.sequential_gradient(hist, slot, scale, PN))
    if n > 200:
        assert not np.array_equal(g, np.ascontiguousarray((hist[slot] * scale[:, None]).T).sum(1))      # a reassociated (pairwise) sum is a different number
    # a narrower parameter count leaves the rest alone and gives the same leading values
    g2 = eg.gradient(hist, slot, scale, 50)
    assert np.array_equal(g2, g[:50])


def test_emulated_history_over_three_plans_keeps_slot_zero_explicit_slots_and_a_stale_tail():
    nu, N = 3, 10
    ctrl = np.tile([-1.0, 1.0], nu)
    hist = np.zeros((N, 36 * nu))
    rng = np.random.default_rng(4)

    def plan(P, fe, seed):
        eps = rng.standard_normal((N, P, nu)); cand = np.zeros((N, P, nu))
        eg.assemble(np.zeros((P, nu)), np.full(P * nu, 0.1), eps, ctrl, cand, hist, 0, 0, fe)
        return eps
    e1 = plan(6, 8, 1)
    assert not hist[0].any() and not hist[8:].any() and np.array_equal(hist[1:8, :18], e1[1:8].reshape(7, 18)) and not hist[:, 18:].any()
    e2 = plan(4, 6, 2)                                                          # fewer spline points, fewer noisy rows
    assert not hist[0].any() and not hist[8:].any()
    assert np.array_equal(hist[1:6, :12], e2[1:6].reshape(5, 12))
    assert np.array_equal(hist[1:6, 12:18], e1[1:6].reshape(5, 18)[:, 12:])     # the stale tail survives a smaller P
    assert np.array_equal(hist[6:8, :18], e1[6:8].reshape(2, 18))               # rows that turned explicit keep the first plan's noise
    e3 = plan(6, 9, 3)
    assert not hist[0].any() and not hist[9:].any() and np.array_equal(hist[1:9, :18], e3[1:9].reshape(8, 18))


def test_emulated_tile_shape_is_the_kernels():
    s = eg.shape()
    assert s["T"] == s["U"] * s["PROD"] and 64 % s["KT"] == 0 and s["PROD"] == 3 * (64 // s["KT"])      # three producer waves of 64 lanes
    assert 2 * s["T"] * s["KT"] * 8 <= 64 * 1024                                # two staging tiles in static LDS


# ----------------------------------------------------------------------------- the loaded product library, host only
def test_new_abi_entry_points_exist_and_leave_the_abi_revision_and_struct_sizes_alone():
    lib = capi.load_engine()
    for sym in ("mjpc_hip_plan_mixed_async", "mjpc_hip_plan_mixed", "mjpc_hip_noise_history_reset", "mjpc_hip_sample_gradient"):
        assert hasattr(lib, sym), sym
    assert lib.mjpc_hip_version() == 4 == capi.ABI_VERSION
    sizes = [lib.mjpc_hip_sizeof_model(), lib.mjpc_hip_sizeof_task(), lib.mjpc_hip_sizeof_plan_input(), lib.mjpc_hip_sizeof_plan_output()]
    assert sizes == [ctypes.sizeof(capi.MjpcHipModel), ctypes.sizeof(capi.MjpcHipTask), ctypes.sizeof(capi.MjpcHipPlanInput),
                     ctypes.sizeof(capi.MjpcHipPlanOutput)]
    assert sizes == SIZEOF_ABI4
    L = cplanner.lib()
    for sym in cplanner.SAMPLE_GRADIENT_C_SYMBOLS:
        assert hasattr(L, sym), sym


SIZEOF_ABI4 = [1152, 136, 160, 104]         # model, task, plan input, plan output at ABI revision 4 (the parent commit's values)


def test_null_and_out_of_range_arguments_are_refused_with_a_message():
    lib = capi.load_engine()
    err = lambda: lib.mjpc_hip_last_error().decode()
    inp = capi.MjpcHipPlanInput(); out = capi.MjpcHipPlanOutput()
    assert lib.mjpc_hip_plan_mixed_async(None, ctypes.byref(inp), 0) != 0 and "invalid argument" in err()
    assert lib.mjpc_hip_plan_mixed(None, None, 0, ctypes.byref(out)) != 0 and "invalid argument" in err()
    assert lib.mjpc_hip_plan_mixed_async(None, ctypes.byref(inp), -1) != 0 and "first_explicit" in err()
    assert lib.mjpc_hip_noise_history_reset(None) != 0 and "mjpc_hip_noise_history_reset" in err()
    g = np.zeros(4); sl = np.zeros(1, np.int32); sc = np.zeros(1)
    assert lib.mjpc_hip_sample_gradient(None, 1, sl.ctypes.data_as(capi.c_int_p), sc.ctypes.data_as(capi.c_double_p), g.ctypes.data_as(capi.c_double_p)) != 0
    assert "mjpc_hip_sample_gradient" in err() and "invalid argument" in err()
