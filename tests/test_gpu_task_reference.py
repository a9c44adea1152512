"""GPU tier of the independent task-residual reference (tests/task_ref.py): the designed batches of tests/task_cases.py through the
one-step kernels (HipBackend.step_batch, one engine per task, set_task between modes, motions and goals), unforced and under the
spill = all and no_model_cache knobs (bit-identical rows), and small plans through the rollout kernels on the engine's own pick and on the
forced dense tier (knob tier = B): residual rows on the engine's OWN states, actions and times against the reference, costs against the
reference's cost of those rows, returns against the mean cost, and the all-norm cost tables at each risk.

MEASURED on an MI355X (worst deviation from the reference; rows relative to max(1, largest |row|), costs and returns per entry relative to
max(1, |entry|)); the CPU tier's figures are in tests/test_task_reference.py:
    one-step rows   quadruped 4.1e-16   tracking 5.0e-16   walk 5.7e-16   interact 3.1e-16     (knob runs: the same bits)
    rollout rows    quadruped 8.9e-16   tracking 2.1e-16   walk 1.3e-15   interact 2.0e-16     (either tier: the same figures)
    costs, returns  own tables 9.3e-15 (tracking; 3.3e-16 elsewhere); all-norm tables 2.14e-14 (tracking at risk 5, where
                    |risk x cost| passes 70: exp() turns one ulp of its argument into that many ulp of the result; 1.9e-15 at the other risks)
The bars are 10 x the worst of these (1.3e-14 on rows, 2.2e-13 on costs given the rows), and under what the Allegro / OP3 GPU tier holds (1e-10 on rows, 1e-12 on costs given the rows).
The forced dense tier engages at N 16 on every model here.
"""
import numpy as np
import pytest

import gradient_planner_cases as gc
import task_cases as tc
from test_task_reference import WARN_FULL, check_coverage, check_plan, rows_dev

pytestmark = pytest.mark.gpu

GPU_MEASURED = dict(rows=1.3e-15, costs=2.2e-14)        # the worst figures above, rounded up to two digits
BAR_ROWS, BAR_COSTS = 10 * GPU_MEASURED["rows"], 10 * GPU_MEASURED["costs"]
assert BAR_ROWS <= 1e-10 and BAR_COSTS <= 1e-12

ONE_STEP = dict(quadruped=[f"quadruped_{x}" for x in tc.QUADRUPED_MODES], tracking=[f"tracking_{k}" for k in tc.TRACK_MOTIONS], walk=["walk"],
                interact=["interact"])


def _one_step_rows(batches):
    """every designed batch of one task on ONE engine, task by task through set_task: ([rows per group], flavour)"""
    from mujoco_mpc_amd.planner import HipBackend
    m, groups = batches[0]
    be = HipBackend(m, groups[0]["task"], max_samples=16, max_horizon=4)
    try:
        rows, full = [], 0
        for m, groups in batches:
            for g in groups:
                be.set_task(g["task"])
                o = be.step_batch(g["X"], g["U"], g["T"], mocap=g["mocap"])
                assert not (o["failure"] & ~WARN_FULL).any(), o["failure"]
                full += int((o["failure"] != 0).sum())
                rows.append(o["residual"])
        return rows, dict(lds=be.lds_bytes(), slab=be.spill_bytes(), full=full)
    finally:
        be.close()


@pytest.mark.parametrize("task", list(ONE_STEP))
def test_one_step_rows_match_the_reference_and_the_knob_runs_match_bit_for_bit(task, debug_knobs):
    batches = [tc.designed(n) for n in ONE_STEP[task]]
    for n, (m, groups) in zip(ONE_STEP[task], batches):
        check_coverage(n, groups)
    rows, flav = _one_step_rows(batches)
    refs = [g["ref"] for _, groups in batches for g in groups]
    worst = max(rows_dev(a, b) for a, b in zip(rows, refs))
    print(f"\n[gpu-task-reference] one-step {task} rows worst={worst:.2e} groups={len(rows)} excluded=0 flavour={flav}")
    assert worst < BAR_ROWS
    for knob, value in (("spill", "all"), ("no_model_cache", "1")):
        debug_knobs(knob, value)
        rows2, flav2 = _one_step_rows(batches)
        debug_knobs(knob, None)
        print(f"[gpu-task-reference] one-step {task} knob {knob}={value} flavour={flav2}")
        assert flav2["slab"] > 0 if knob == "spill" else flav2["lds"] < flav["lds"]        # the knob took effect
        for a, b in zip(rows, rows2):
            assert np.array_equal(a, b), knob


def _plan(be, pi, N, H):
    out = be.plan(state=pi["state"], mocap=pi["mocap"], time=pi["time"], knot_times=pi["knot_times"], knot_values=pi["knot_values"],
                  interpolation=pi["interp"], num_trajectory=N, horizon=H, sigma=pi["sigma"], noise_eps=pi["eps"], noise_sel=pi["sel"])
    allc = be.fetch_all(N, H, len(pi["knot_times"]))
    return dict(allc, returns=out["returns"], failure=out["failure"], winner=out["winner"])


ALL_NORMS = ("quadruped_walk", "tracking_0")


@pytest.mark.parametrize("dense", [False, True], ids=["own_pick", "tier_B"])
@pytest.mark.parametrize("name", tc.PLANS)
def test_rollout_rows_costs_and_returns_match_the_reference(name, dense, debug_knobs):
    """N 16, H 12, the task's own P and spline, explicit Philox noise; every candidate fetched"""
    from mujoco_mpc_amd.planner import HipBackend
    m, task, d = tc.plan_task(name)
    N, H = 16, 12
    pi = tc.plan_inputs(m, d, N, H)
    if dense:
        debug_knobs("tier", "B")
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = _plan(be, pi, N, H)
        tier, slab = be.dense_tier(), be.spill_bytes()
        print(f"\n[gpu-task-reference] rollout {name} dense_tier={tier} spill_bytes={slab} lds={be.lds_bytes()}")
        assert tier[1] == dense and (tier[0] > 0) >= dense
        assert not out["failure"].any() and np.ptp(out["returns"]) > 0
        assert out["winner"] == int(np.argmin(out["returns"]))
        tr = check_plan(f"gpu {name} {'tier B' if dense else 'own pick'}", m, task, pi["mocap"], out, BAR_ROWS, BAR_COSTS)
    finally:
        be.close()
    if name not in ALL_NORMS:
        return
    for k, risk in enumerate(tc.RISKS):                                            # (a longer cost table needs an engine of its own:
        t = gc.regroup(task, "all", risk, seed=k)                                  # set_task refuses a task that grew beyond create()'s)
        be = HipBackend(m, t, max_samples=N, max_horizon=H)
        try:
            o2 = _plan(be, pi, N, H)
            assert be.dense_tier()[1] == dense
        finally:
            be.close()
        assert np.array_equal(o2["residual"], out["residual"])                     # the rows do not depend on the cost table
        c = tr.cost(o2["residual"], t)
        dc, dret = gc.dev(o2["costs"], c), gc.dev(o2["returns"], c.mean(1))
        print(f"[gpu-task-reference] rollout {name} all norms risk={risk} costs={dc:.2e} returns={dret:.2e} largest={np.abs(c).max():.3g}")
        assert np.isfinite(c).all() and dc < BAR_COSTS and dret < BAR_COSTS
