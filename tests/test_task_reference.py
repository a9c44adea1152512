"""CPU tier of the independent task-residual reference (tests/task_ref.py) for Quadruped flat (2), Humanoid tracking (4), Humanoid
walk (6) and Humanoid interact (15): the kernel source in its 1-lane emulation (residuals.h through emu_transition_lib.step_batch and
emu_lib.plan) and the oracle's restatement (oracle/task.c) against rows written from the reference's own sources, on the designed
batches of tests/task_cases.py; costs with every norm type and the risk transform against closed forms; returns = mean cost.

Every test asserts that the branches it is there for were entered.  The designed batches exclude 0 rows; rows on the emulation's own
rollout states may be skipped where the reference's margin to a discontinuity is under 1e-9 (at most 1 %, count printed).

MEASURED here (worst deviation from the reference; rows relative to max(1, largest |row|) of the batch, costs and returns per entry
relative to max(1, |entry|)), emulation / oracle on the designed batches, then the small plans:
    quadruped    rows 4.8e-16 / 4.9e-16     plan rows 4.4e-16     costs, returns: own table 0, all norms 2.0e-15
    tracking     rows 4.5e-16 / 1.2e-15     plan rows 2.3e-16     own table 4.2e-15, all norms 1.43e-14
    walk         rows 5.7e-16 / 1.3e-15     plan rows 6.5e-16     own table 1.7e-16, all norms 1.9e-15
    interact     rows 4.3e-16 / 6.7e-16     plan rows 2.4e-16     own table 2.2e-16, all norms 1.44e-14
The cost figures grow with |risk x cost|: at risk 5 the interact and tracking plans reach risk x cost near 90, and exp() turns one
ulp of its argument into that many ulp of the result.  BARS = 10 x the worst: 1.4e-14 on rows, 1.5e-13 on costs given the rows.
"""
import numpy as np
import pytest

import emu_lib
import emu_transition_lib as et
import gradient_planner_cases as gc
import oracle_lib as ol
import task_cases as tc
from task_ref import as_int

CPU_MEASURED = dict(rows=1.4e-15, costs=1.5e-14)      # the worst figures above, rounded up to two digits
BAR_ROWS, BAR_COSTS = 10 * CPU_MEASURED["rows"], 10 * CPU_MEASURED["costs"]
WARN_RAY, WARN_FULL = 32, 8 | 16


def rows_dev(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def _entered(groups, key):
    return np.concatenate([np.asarray(g["entered"][key]).reshape(len(g["X"]), -1) for g in groups])


def check_coverage(name, groups):
    """the branches the batch was designed to enter, from what the reference recorded"""
    if name.startswith("quadruped_"):
        mode = tc.QUADRUPED_MODES.index(name[10:])
        I = lambda g: [int(x) for x in g["task"]["int_data"]]                    # noqa: E731
        P = lambda g, k: g["task"]["parameters"][I(g)[k]]                        # noqa: E731
        assert all(I(g)[-1] == mode for g in groups) and sum(len(g["X"]) for g in groups) == 128
        assert {x for g in groups for x in g["places"]} == set(tc.PLACES)
        assert {float(P(g, 13)) for g in groups} == set(tc.DUTY) and {float(g["task"]["dbl_data"][16]) for g in groups} == set(tc.PHASE_VELOCITY)
        assert any(P(g, 12) == 0.0 for g in groups)                              # amplitude exactly 0: step ? ... : 0 takes its zero arm
        st = _entered(groups, "stepped")
        assert st.any() and (~st).any()
        if mode == 1:
            assert set(_entered(groups, "gait").ravel()) == {2}
            assert {as_int(P(g, 10)) for g in groups} == {0, 1}               # both biped types
        else:
            assert set(_entered(groups, "gait").ravel()) == {0, 1, 2, 3, 4}
        if mode == 2:
            assert {float(g["task"]["dbl_data"][7]) for g in groups} == set(tc.ANGVEL)
            w = _entered(groups, "walk_turning")
            assert w.any() and (~w).any()
        if mode == 3:
            assert _entered(groups, "scramble_above").any() and _entered(groups, "scramble_below").any()
        if mode == 4:
            assert set(_entered(groups, "flip_phase").ravel()) == {0, 1, 2, 3, 4}
            assert {as_int(P(g, 9)) for g in groups} == {0, 1}                # both flip directions
            on = np.concatenate([np.abs((g["T"] - g["task"]["dbl_data"][0])[:, None] - np.array(tc.flip_bounds(g["task"]["dbl_data"]))[None]) == 0 for g in groups])
            assert on.any(0).all() and on.sum() >= 16                            # each of the four boundaries hit exactly, several times
    elif name.startswith("tracking_"):
        e = groups[0]["entered"]
        length = int(groups[0]["task"]["int_data"][2])
        assert e["clamp_low"].sum() >= 2 and e["clamp_high"].sum() >= 4 and e["k1_clamped"].sum() >= 8 and e["on_key"].sum() >= 16
        assert (e["k0"] == length - 2).sum() >= 4 and (e["k0"] == length - 1).sum() >= 8
        assert (e["k0"] < 0).any() == (int(groups[0]["task"]["int_data"][1]) > 0)      # before the start: the keys of the motion stored before
    elif name == "walk":
        e = groups[0]["entered"]
        assert e["length_negative"].sum() >= 4 and (~e["length_negative"]).any() and e["forward_guard"].sum() == 4 and e["clamped"].any() and (~e["clamped"]).any()
    else:
        assert {(g["mode"], g["facing"]) for g in groups} == {(k, f) for k in range(4) for f in tc.INTERACT_FACING}
        for g in groups:
            assert g["entered"]["pairs_active"] == [True, True, False, False, True]
            assert g["entered"]["facing"].all() == (g["facing"] != "none")
            if g["facing"] != "none":
                assert g["entered"]["facing_guard"].all() == (g["facing"] == "above") and g["entered"]["facing_guard"].any() == (g["facing"] == "above")


@pytest.mark.parametrize("name", tc.DESIGNED)
def test_emulated_kernel_rows_match_the_reference_on_the_designed_batches(name):
    """emu_transition_lib.step_batch, group by group: every row of every case within BAR_ROWS; no ray missed; nothing excluded"""
    m, groups = tc.designed(name)
    check_coverage(name, groups)
    worst, full = 0.0, 0
    for g in groups:
        _, res, fail = et.step_batch(m, g["task"], g["X"], g["U"], g["T"], g["mocap"])
        assert not (fail & ~WARN_FULL).any(), fail                                 # (a full contact buffer in the step behind the row is no concern of the row)
        full += int((fail != 0).sum())
        worst = max(worst, rows_dev(res, g["ref"]))
    print(f"\n[task-reference] {name} emulation rows worst={worst:.2e} excluded=0 steps_with_full_buffers={full}")
    assert worst < BAR_ROWS


@pytest.mark.parametrize("name", tc.DESIGNED)
def test_oracle_rows_match_the_reference_on_the_designed_batches(name):
    """oracle/task.c held to the same rows: the sensordata of one forward pass per case"""
    m, groups = tc.designed(name)
    worst = 0.0
    nq, nv = m["nq"], m["nv"]
    for g in groups:
        o = ol.Oracle(m, g["task"])
        for i in range(len(g["X"])):
            f = o.forward(g["X"][i, :nq], g["X"][i, nq:nq + nv], g["U"][i], g["mocap"], time=float(g["T"][i]))
            assert not (f["warning"] & WARN_RAY) and f["unsupported"] == 0
            worst = max(worst, rows_dev(f["sensordata"], g["ref"][i]))
    print(f"\n[task-reference] {name} oracle rows worst={worst:.2e}")
    assert worst < BAR_ROWS


def _plan(m, task, pi, N, H):
    return emu_lib.plan(m, task, pi["state"], pi["mocap"], pi["time"], pi["knot_times"], pi["knot_values"], pi["interp"], N, H, sigma=pi["sigma"],
                        noise_eps=pi["eps"], noise_sel=pi["sel"])


def check_plan(label, m, task, mocap, out, bar_rows, bar_costs):
    """rows on the plan's own states against the reference (margin under 1e-9: skipped, at most 1 %), costs against the reference's
    cost of the plan's rows, returns against the mean cost"""
    r, keep, tr = tc.rollout_reference(m, task, mocap, out)
    skipped = int((~keep).sum())
    print(f"\n[task-reference] {label} rollout rows skipped={skipped} of {keep.size}")
    assert skipped <= 0.01 * keep.size
    dr = rows_dev(out["residual"][keep], r[keep])
    c = tr.cost(out["residual"])
    dc = gc.dev(out["costs"], c)
    dret = gc.dev(out["returns"], c.mean(1))
    print(f"[task-reference] {label} rows={dr:.2e} costs={dc:.2e} returns={dret:.2e}")
    assert dr < bar_rows and dc < bar_costs and dret < bar_costs
    return tr


@pytest.mark.parametrize("name", tc.PLANS)
def test_emulated_small_plans_rows_costs_and_returns(name):
    """N 4, H 6 per quadruped mode and per humanoid task, then the same plan with the all-norm cost tables at each risk"""
    m, task, d = tc.plan_task(name)
    N, H = 4, 6
    pi = tc.plan_inputs(m, d, N, H)
    out = _plan(m, task, pi, N, H)
    assert not out["failure"].any() and np.ptp(out["returns"]) > 0
    tr = check_plan(name, m, task, pi["mocap"], out, BAR_ROWS, BAR_COSTS)
    seen = set()
    for k, risk in enumerate(tc.RISKS):
        t = gc.regroup(task, "all", risk, seed=k)
        o2 = _plan(m, t, pi, N, H)
        assert np.array_equal(o2["residual"], out["residual"])                     # the rows do not depend on the cost table
        c = tr.cost(o2["residual"], t)
        seen |= tr.norms_entered
        dc, dret = gc.dev(o2["costs"], c), gc.dev(o2["returns"], c.mean(1))
        print(f"[task-reference] {name} all norms risk={risk} costs={dc:.2e} returns={dret:.2e} largest={np.abs(c).max():.3g}")
        assert np.isfinite(c).all() and dc < BAR_COSTS and dret < BAR_COSTS
    assert seen == {-1, 0, 1, 2, 3, 5, 6, 7, (8, True), (8, False)}
