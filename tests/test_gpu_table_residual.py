"""GPU tier of the table-driven residual (MJPC_TASK_TABLE = 19): through HipBackend, a table task against its built-in twin on the
same inputs on every kernel family, sampled rows against the independent reference tests/table_ref.py on the engine's own states,
mjpc_hip_set_task with tables, and a closed loop through the testspeed harness."""
import numpy as np
import pytest

import oracle_lib as ol
import table_ref as tr
from mujoco_mpc_amd.modelgen import TABLE_TASKS, ResidualTable
from test_table_residual import BUILTIN, plan_inputs

pytestmark = pytest.mark.gpu

TRAJ = ("states", "actions", "times", "knots")
PAIRS = 384          # (candidate, step) pairs whose rows are recomputed by table_ref


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _engine(m, task, st, mocap, N, H, kt, kv, d, eps, sel):
    from mujoco_mpc_amd.planner import HipBackend
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        out = be.plan(state=st, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=d["interp"], num_trajectory=N,
                      horizon=H, sigma=d["sigma"], noise_eps=eps, noise_sel=sel)
        return out, be.fetch_all(N, H, len(kt)), dict(lds=be.lds_bytes(), slab=be.spill_bytes(), dense=be.dense_tier())
    finally:
        be.close()


# (task, candidates, dense tier expected): generic cached kernels (walker, fingers with the noslip pass, swimmer), cached<2>
# (particle_fixed), cached<18> and its dense tier (quadruped_hill), <27> both tiers (humanoid_stand), direct<33> and the hand's dense
# tier (shadow_hand)
CASES = [("walker", 64, False), ("fingers", 64, False), ("swimmer", 32, False), ("particle_fixed", 64, False),
         ("quadruped_hill", 256, False), ("quadruped_hill", 512, True), ("humanoid_stand", 256, False), ("humanoid_stand", 1024, True),
         ("shadow_hand", 256, False), ("shadow_hand", 2048, True)]


def _compare(name, N, dense, spill=False):
    m, tb, d = BUILTIN[name]()
    m2, tt, _ = TABLE_TASKS[name]()
    st, mocap, kt, kv, eps, sel, H = plan_inputs(name, m, d, N, seed=11)
    oa, a, fa = _engine(m, tb, st, mocap, N, H, kt, kv, d, eps, sel)
    ob, b, fb = _engine(m2, tt, st, mocap, N, H, kt, kv, d, eps, sel)
    print(name, N, "flavours built-in / table:", fa, fb)
    # a candidate whose rollout stops (a full contact buffer among 256+ noisy candidates on the terrain) stops in both runs alike:
    # the dynamics never read the residual.  Its rows behind the stop are not written, so the arrays are compared on the others
    assert np.array_equal(oa["failure"], ob["failure"])
    ok = oa["failure"] == 0
    print(name, N, "failed candidates:", int((~ok).sum()))
    assert ok.mean() > 0.9
    a = {k: v[ok] for k, v in a.items()}; b = {k: v[ok] for k, v in b.items()}
    if dense:
        assert fa["dense"][0] > 0 and fa["dense"][1] and fb["dense"][0] > 0 and fb["dense"][1], (fa, fb)
    if spill:
        assert fa["slab"] > 0 and fb["slab"] > 0
    for k in TRAJ:
        assert np.array_equal(a[k], b[k]), k
    for k, x, y in (("residual", b["residual"], a["residual"]), ("costs", b["costs"], a["costs"]), ("returns", ob["returns"], oa["returns"])):
        err = _rel(x, y)
        print(name, N, k, "table against built-in:", err)
        assert err < 1e-12, (k, err)
    assert oa["winner"] == ob["winner"] and ob["winner"] == int(np.argmin(ob["returns"]))
    assert np.ptp(ob["returns"]) > 0
    rng = np.random.default_rng(5)
    n = int(ok.sum())
    k = rng.choice(n * H, min(PAIRS, n * H), replace=False)
    c, t = k // H, k % H
    r = tr.TableRef(m, tt).residual(b["states"][c, t], b["actions"][c, t], mocap)
    err = _rel(b["residual"][c, t], r)
    print(name, N, "sampled rows against table_ref:", err)
    assert err < 1e-10, err


@pytest.mark.parametrize("name,N,dense", CASES, ids=[f"{n}-{N}" for n, N, _ in CASES])
def test_table_against_builtin_on_each_kernel_family(name, N, dense):
    """built-in against table, all candidates: states / actions / times / knots bit for bit, residual rows, costs and returns at
    1e-12, winner exact; 384 sampled (candidate, step) rows against table_ref at 1e-10; the dense tier ran where the case names it"""
    _compare(name, N, dense)


def test_table_against_builtin_on_the_spill_flavour(debug_knobs):
    """allegro with every eligible block forced into the HBM slab (knob spill = all)"""
    debug_knobs("spill", "all")
    _compare("allegro", 64, False, spill=True)


def _walker_variant(m, longer=False):
    """a second table of the walker's size: the same sources in the same shapes, other coefficients and another component of the torso's axis;
    longer: one more term in the first block"""
    t = ResidualTable(m)
    t.sum(2.0 * t.ctrl() + 0.5 * t.qvel()[:6] if longer else 2.0 * t.ctrl())
    t.sum(t.pos("xbody", "torso")[2] - t.param(0))
    t.sum(t.zaxis("xbody", "torso")[0] - 1.0)
    t.sum(-1.0 * t.subtree_linvel("torso")[0] + t.param(1))
    return t


def test_set_task_installs_a_new_goal_and_a_new_table_and_refuses_a_longer_one():
    from mujoco_mpc_amd.planner import HipBackend
    m, task, d = TABLE_TASKS["walker"]()
    N = 16
    st, mocap, kt, kv, eps, sel, H = plan_inputs("walker", m, d, N, seed=3)
    kw = dict(state=st, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=d["interp"], num_trajectory=N, horizon=H,
              sigma=d["sigma"], noise_eps=eps, noise_sel=sel)
    cost = dict(terms=[(6, 0, 0.1), (1, 0, 10.0), (1, 0, 3.0), (1, 0, 1.0)])

    def rows(be, t):
        out = be.plan(**kw)
        allc = be.fetch_all(N, H, len(kt))
        r = tr.TableRef(m, t).residual(allc["states"].reshape(N * H, -1), allc["actions"].reshape(N * H, -1), mocap).reshape(allc["residual"].shape)
        assert _rel(allc["residual"], r) < 1e-10
        return out, allc

    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    try:
        o0, a0 = rows(be, task)
        moved = dict(task, parameters=np.array([0.9, 1.5]))                 # the PARAM goals move, the table stays
        be.set_task(moved)
        o1, a1 = rows(be, moved)
        assert np.array_equal(a0["states"], a1["states"])
        diff = np.flatnonzero((a0["residual"] != a1["residual"]).any((0, 1)))
        assert list(diff) == [6, 8] and not np.array_equal(o0["returns"], o1["returns"])
        other = _walker_variant(m).task(parameters=[1.2, 0.0], traces=[(int(task["trace_objtype"][0]), int(task["trace_objid"][0]))], **cost)
        assert other["num_int"] == task["num_int"] and other["num_dbl"] == task["num_dbl"]
        be.set_task(other)
        o2, a2 = rows(be, other)
        assert np.array_equal(a2["residual"][..., :6], 2.0 * a0["residual"][..., :6]) and not np.array_equal(a2["residual"][..., 7], a0["residual"][..., 7])
        longer = _walker_variant(m, longer=True).task(parameters=[1.2, 0.0], traces=[(int(task["trace_objtype"][0]), int(task["trace_objid"][0]))], **cost)
        assert longer["num_int"] > task["num_int"]
        with pytest.raises(RuntimeError, match="grew beyond"):
            be.set_task(longer)
        bad = dict(other, int_data=np.array(other["int_data"], np.int32))
        bad["int_data"][3] = 9                                              # unknown operation: refused by the validation
        with pytest.raises(RuntimeError, match="block 0"):
            be.set_task(bad)
        be.task = other
        o3, a3 = rows(be, other)                                            # the engine still prices with the last good table
        assert np.array_equal(o3["returns"], o2["returns"]) and np.array_equal(a3["residual"], a2["residual"])
    finally:
        be.close()


def test_closed_loop_walker_table_ends_where_the_builtin_ends():
    """cplanner.testspeed with the walker's numerics (3 cubic spline points, exploration 0.5, 10 trajectories, horizon 0.8 s),
    40 steps, same seed: no failure, and the final state equals the built-in walker's bit for bit (the state only depends on
    which candidate wins each plan)."""
    from mujoco_mpc_amd import cplanner
    res = {}
    for kind, gen in (("builtin", BUILTIN["walker"]), ("table", TABLE_TASKS["walker"])):
        m, task, d = gen()
        num = dict(sampling_spline_points=3, sampling_exploration=0.5, sampling_trajectories=10, sampling_representation=2)
        p = cplanner.SamplingPlanner()
        p.Initialize(m, task, num, max_samples=10, max_horizon=d["horizon"])
        p.Reset(d["horizon"])
        res[kind] = cplanner.testspeed(p, d["state"], None, horizon=d["horizon"], steps_per_planning_iteration=1, total_time=40 * m["timestep"])
        p.close()
        assert not res[kind]["failure"] and np.isfinite(res[kind]["average_cost"])
    print("walker closed loop: average cost built-in", res["builtin"]["average_cost"], "table", res["table"]["average_cost"])
    assert np.ptp(res["table"]["state"] - d["state"]) > 0
    assert np.array_equal(res["builtin"]["state"], res["table"]["state"])
    assert _rel(res["table"]["cost_per_step"], res["builtin"]["cost_per_step"]) < 1e-12
