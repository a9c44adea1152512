#!/usr/bin/env python3
"""Host wall time of the iLQG backward pass on a model's own matrices: mjpc_hip_ilqg_backward_pass (device: uploads, one kernel, one download)
against the host C++ iLQGBackwardPass::RiccatiRegularized on the same matrices (what a user without the kernel would run after downloading
them), and mjpc_hip_trajectory_ilqg (fused: transition_fd, cost derivatives with Hessians, backward pass, one download) against the composed
path (the three calls with their matrices downloaded in between).  The paths alternate in one process, through preallocated arrays.

usage: tools/time_ilqg_backward.py [--model quadruped|humanoid_track|...] [--T 36] [--limits 0|1] [--reg-type 0] [--calls 5] [--passes 2]
                                   [--only device|host|fused|composed]      (one path alone: for a profiler run)
Prints one line per pass and path: median (min - max) in ms, and the backward pass's time per knot.  DESIGN section 8g holds the recorded
figures."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mujoco_mpc_amd import derivatives                             # noqa: E402
from mujoco_mpc_amd.modelgen import REGISTRY                       # noqa: E402
from mujoco_mpc_amd.planner import HipBackend                      # noqa: E402
from time_trajectory_gradient import scattered, stats              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="quadruped"); ap.add_argument("--T", type=int, default=36); ap.add_argument("--limits", type=int, default=1)
    ap.add_argument("--reg-type", type=int, default=0); ap.add_argument("--calls", type=int, default=5); ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    m, task, d = REGISTRY[a.model]()
    be = HipBackend(m, task, max_samples=4096, max_horizon=2)
    T, nd, nu = a.T, 2 * m["nv"] + m["na"], m["nu"]
    X, U, Tm = scattered(m, d, T)
    mocap = np.asarray(d["mocap"], float) if len(d["mocap"]) else None
    res = be.step_batch(X, U, Tm, mocap=mocap)["residual"]
    kw = dict(regularization_type=a.reg_type, action_limits_on=a.limits)
    rng = np.asarray(m["actuator_ctrlrange"], float).reshape(-1, 2).copy()
    rng[np.ravel(m["actuator_ctrllimited"]) == 0] = (-np.inf, np.inf)
    bp = derivatives.ILQGBackwardPass(nd, nu, T)

    def derivs():
        fd = be.transition_fd(X, U, Tm, mocap=mocap, eps=1e-6, last_is_terminal=True)
        cd = be.cost_derivatives(res, fd["C"], fd["D"], last_is_terminal=True, hessians=True)
        return fd, [fd["A"], fd["B"], cd["cx"], cd["cu"], cd["cxx"], cd["cxu"], cd["cuu"], U, rng]

    fd, mats = derivs()
    assert not fd["failure"].any(), "a failed evaluation: not a timing state"

    def device():
        return be.ilqg_backward_pass(*mats, **kw)

    def host():
        bp.regularization = (1.0, 1.0, 2.0)
        return bp.riccati_host(*mats, **kw)

    def fused():
        return be.trajectory_ilqg(X, U, Tm, res, mocap=mocap, eps=1e-6, **kw)

    def composed():
        return be.ilqg_backward_pass(*derivs()[1], **kw)

    def timed(fn):
        t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

    g, h, f = device(), host(), fused()                           # warm-up, and the three agree
    for k in ("k", "K", "Vx", "Vxx", "dV"):
        assert np.array_equal(g[k], h[k]) and np.array_equal(g[k], f[k]), k
    print(f"{a.model} T={T} nd={nd} nu={nu} limits={a.limits} regularization_type={a.reg_type} status={list(g['status'])} "
          f"regularization={g['regularization']:g}")
    for p in range(a.passes):
        for name, fn in (("device", device), ("host", host), ("fused", fused), ("composed", composed)):
            if a.only in ("", name):
                ts = [timed(fn) for _ in range(a.calls)]
                per = "  %.1f us per knot" % (1e6 * np.median(ts) / (T - 1)) if name in ("device", "host") else ""
                print(f"pass {p + 1} {name:9s} {stats(ts)}{per}")
    be.close()


if __name__ == "__main__":
    main()
