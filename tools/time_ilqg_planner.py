#!/usr/bin/env python3
"""Device time of the feedback-policy rollout (mjpc_hip_plan_feedback) beside the open-loop rollout of the same N x H with explicit candidates
(mjpc_hip_plan) on the same engine, alternating; the resampling kernel's time; and one iLQGPlanner::OptimizePolicy split into its parts.

usage: tools/time_ilqg_planner.py [--model quadruped|humanoid_track|...] [--N 32] [--H 36] [--calls 5] [--passes 2] [--no-planner]
The rollout times are mjpc_hip_kernel_time's (hipEvents around the rollout kernel); each figure is the median of --calls launches with min and
max.  The difference between the two medians, over H - 1 steps, is what the feedback head costs per step.  DESIGN section 8h holds the
recorded figures."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_mpc_amd import capi, cplanner                          # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY                       # noqa: E402
from mujoco_mpc_amd.planner import HipBackend                      # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v, float))
    return f"{np.median(v):9.1f} ({v[0]:.1f} - {v[-1]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--N", type=int, default=32); ap.add_argument("--H", type=int, default=36)
    ap.add_argument("--calls", type=int, default=5); ap.add_argument("--passes", type=int, default=2); ap.add_argument("--no-planner", action="store_true")
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    N, H = a.N, a.H
    nu, nd = m["nu"], 2 * m["nv"] + m["na"]
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    x0 = np.asarray(d["state"], float)
    be = HipBackend(m, task, max_samples=N, max_horizon=H)
    rng = np.random.default_rng(0)
    cr = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2)
    h = float(m["timestep"])
    times = np.cumsum(np.r_[0.0, np.full(H - 1, h)])
    u = 0.5 * (cr[:, 0] + cr[:, 1]) + 0.05 * 0.5 * (cr[:, 1] - cr[:, 0]) * rng.uniform(-1, 1, (H, nu))
    P = min(H, 36)
    kt = times[:P] if P == H else np.linspace(0.0, times[-1], P)
    kv = u[:P]
    cand = np.tile(kv[None], (N, 1, 1))
    nom = be.plan(state=x0, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=0, num_trajectory=N, horizon=H, sigma=(0.0, 0.0),
                  candidate_knots=cand)
    assert not nom["failure"].any(), "the nominal rollout failed: not a timing state"
    K = 0.02 * rng.standard_normal((H, nu, nd)); k = 0.01 * rng.standard_normal((H, nu))
    steps = np.r_[np.exp(np.linspace(np.log(1e-3), 0.0, N - 1)), 0.0]

    def open_loop():
        be.plan(state=x0, mocap=mocap, time=0.0, knot_times=kt, knot_values=kv, interpolation=0, num_trajectory=N, horizon=H, sigma=(0.0, 0.0), candidate_knots=cand)
        return be.kernel_time()[1], 0.0

    def feedback(mode):
        def run():
            o = be.plan_feedback(x0, 0.0, H, nom["times"], nom["states"], nom["actions"], K, steps if mode == 0 else np.zeros(N),
                                 np.ones(N) if mode == 0 else steps, action_improvement=k, mode=mode, representation=1, mocap=mocap)
            assert not o["failure"].any()
            return be.kernel_time()[1], o["resample_time_us"]
        return run
    paths = [("open loop (mjpc_hip_plan)", open_loop), ("feedback, indexed", feedback(0)), ("feedback, time (linear)", feedback(1))]
    for _, f in paths:
        f()                                     # warm-up: first launches, buffers
    print(f"{a.model}: N = {N}, H = {H}, nd = {nd}, nu = {nu}; rollout kernel time in us, median (min - max) of {a.calls}")
    med = {}
    for p in range(a.passes):
        acc = {name: [] for name, _ in paths}; res = []
        for _ in range(a.calls):
            for name, f in paths:               # alternating
                t, r = f()
                acc[name].append(t)
                if name.endswith("(linear)"):
                    res.append(r)
        for name, _ in paths:
            print(f"pass {p}  {name:28s} {stats(acc[name])}")
            med.setdefault(name, []).append(np.median(acc[name]))
        print(f"pass {p}  {'resampling kernel':28s} {stats(res)}")
    base = np.mean(med[paths[0][0]])
    for name, _ in paths[1:]:
        print(f"{name}: {np.mean(med[name]) - base:+.1f} us per rollout against open loop, {(np.mean(med[name]) - base) / (H - 1):+.3f} us per step")
    be.close()
    if a.no_planner:
        return
    pl = cplanner.iLQGPlanner()
    pl.Initialize(m, task, dict(ilqg_num_rollouts=N), max_samples=N, max_horizon=H)
    pl.Reset(H)
    pl.SetState(x0, mocap, None, 0.0)
    rows = []
    for i in range(a.calls + 1):
        pl.OptimizePolicy(H)
        if i:
            rows.append(pl.timings())
    print("one OptimizePolicy, host wall time in us, median (min - max):")
    for key in ("nominal_us", "derivative_us", "rollouts_us", "policy_update_us", "resample_kernel_us", "rollout_kernel_us"):
        print(f"  {key:20s} {stats([r[key] for r in rows])}")
    print("  values:", pl.values())


if __name__ == "__main__":
    main()
