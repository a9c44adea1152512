#!/usr/bin/env python3
"""One iLQSPlanner::OptimizePolicy split into its parts, per branch, and the host time of the spline fit with a cold and a warm operator cache.

usage: tools/time_ilqs_planner.py [--model quadruped|humanoid_track|...] [--N 32] [--H 36] [--P 6] [--sigma 0.05] [--calls 5]
Per repetition the planner is reset and called three times from the same state without sampling noise, so that no candidate beats member 0:
the first call runs sampling and the iteration seeded from sampling's member 0, the second and third convert iLQG's nominal first (when iLQG
took over), the second with a cold cache (Reset clears it), the third with a warm one.  Then it is reset and called once with noise: sampling
alone when a candidate improved.  Calls are sorted by the branch the planner reports, not by position.  Host wall times in microseconds, median
(min - max); `sampling` is the sampling member's rollouts timer (its whole batch, noise included) plus its policy update.  DESIGN section 8i
holds the recorded figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_mpc_amd import cplanner                                # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY                       # noqa: E402

PARTS = ("total", "nominal", "fit", "sampling", "derivatives", "rollouts", "update")


def stats(v):
    v = np.sort(np.asarray(v, float))
    return f"{np.median(v):9.1f} ({v[0]:.1f} - {v[-1]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--N", type=int, default=32); ap.add_argument("--H", type=int, default=36)
    ap.add_argument("--P", type=int, default=6); ap.add_argument("--sigma", type=float, default=0.05); ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    N, H = a.N, a.H
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    x0 = np.asarray(d["state"], float)
    pl = cplanner.iLQSPlanner()
    pl.Initialize(m, task, dict(sampling_trajectories=N, sampling_representation=2, sampling_spline_points=a.P, sampling_exploration=0.0,
                                ilqg_num_rollouts=N), max_samples=N, max_horizon=H)
    rows = {}

    def call(sigma):
        pl.set_noise_exploration(sigma)
        pl.SetState(x0, mocap, None, 0.0)
        t0 = time.perf_counter()
        pl.OptimizePolicy(H)
        total = (time.perf_counter() - t0) * 1e6
        v, tm = pl.values(), pl.timings()
        if v["returned_early"]:
            branch = ("conversion + " if v["converted"] else "") + "sampling only (early return)"
        elif v["converted"]:
            branch = "conversion (%s cache) + sampling + iteration" % ("cold" if tm["fit_cache_miss"] else "warm")
        else:
            branch = "sampling + iteration seeded from member 0"
        s, q = tm["sampling"], tm["ilqg"]
        r = dict(total=total, nominal=q["nominal_us"] if v["converted"] else 0.0, fit=tm["fit_us"] if v["converted"] else 0.0,
                 sampling=s["rollouts_us"] + s["policy_update_us"], derivatives=q["derivative_us"], rollouts=q["rollouts_us"], update=q["policy_update_us"])
        rows.setdefault(branch, []).append(r)

    pl.Reset(H); call(0.0); call(a.sigma)          # warm-up: first launches, buffers
    rows.clear()
    for _ in range(a.calls):
        pl.Reset(H)
        for _ in range(3):
            call(0.0)
        pl.Reset(H)
        call(a.sigma)
    print(f"{a.model}: sampling N = {N}, iLQG N = {N}, H = {H}, P = {a.P} (cubic), nu = {m['nu']}; one OptimizePolicy, host wall time in us, median (min - max)")
    for branch, rs in rows.items():
        print(f"{branch}: {len(rs)} call(s)")
        for key in PARTS:
            print(f"  {key:12s} {stats([r[key] for r in rs])}")
    print("values of the last call:", pl.values())


if __name__ == "__main__":
    main()
